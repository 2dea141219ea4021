"""Shared by the EMA-codebook tests and by tests/golden/codebook_train/make_golden_codebook.py: the statements of reference
mebt/modules/codebook.py:25-46,66-89 on plain tensors in a chosen dtype (float64: the twin the kernels are held to; float32: the
reference's own arithmetic on the CPU), the code statistics without the one-hot matrix, and the fixture loader.  Test infrastructure
only: the product never calls it."""
import glob
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codebook_train")
STEPS = 4                     # recorded training forwards: three followed by an SGD step, and the one after the third


def load_fixture():
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN_DIR, "codebook_golden*.npz"))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def sums_twin(ids, z, n_codes):
    """ids int64 [M], z [M, d] -> float64 (n_total [n_codes], encode_sum [n_codes, d], abs_sum [n_codes, d] = the same sum over |z|);
    ids outside [0, n_codes) are skipped (codebook.py:68-69 without the one-hot matrix)"""
    ids = ids.reshape(-1).cpu()
    z = z.reshape(ids.numel(), -1).cpu().double()
    ok = (ids >= 0) & (ids < n_codes)
    kept, rows = ids[ok], z[ok]
    n_total = torch.bincount(kept, minlength=n_codes).double()
    encode_sum = torch.zeros(n_codes, z.shape[1], dtype=torch.float64).index_add_(0, kept, rows)
    abs_sum = torch.zeros(n_codes, z.shape[1], dtype=torch.float64).index_add_(0, kept, rows.abs())
    return n_total, encode_sum, abs_sum


def restart_rows_twin(z, src, noise):
    """`_k_rand` of codebook.py:25-32,41,83 in z's dtype: row j = z[src[j] mod M] + noise[j] * std.  In float32 these are the reference's
    own two roundings (the product, then the sum); noise None: the plain rows (M >= n_codes)."""
    M, d = z.shape
    rows = z[src % M]
    if noise is None:
        return rows.clone()
    std = 0.01 / np.sqrt(d)                        # numpy float64, as in `_tile`; torch rounds it to the tensor's dtype
    return rows + noise.to(z.dtype) * std


def ema_statements(N, z_avg, n_total, encode_sum, k_rand, restart_thres, no_random_restart):
    """codebook.py:74-80,87-89, statement by statement, in the dtype of the tensors given (N and z_avg are updated in place)
    -> (embeddings, usage [n_codes] bool)"""
    n_codes = N.shape[0]
    N.mul_(0.99).add_(n_total, alpha=0.01)
    z_avg.mul_(0.99).add_(encode_sum, alpha=0.01)
    n = N.sum()
    weights = (N + 1e-7) / (n + n_codes * 1e-7) * n
    emb = z_avg / weights.unsqueeze(1)
    usage = (N.view(n_codes, 1) >= restart_thres)
    if not no_random_restart:
        u = usage.to(emb.dtype)
        emb.mul_(u).add_(k_rand * (1 - u))
    return emb, usage.view(-1)


def ema_reference(N, z_avg, n_total, encode_sum, k_rand, restart_thres, no_random_restart):
    """-> {dtype: (N, z_avg, embeddings, usage)} for float32 (the reference's arithmetic) and float64 (the twin), from the same fp32 inputs"""
    out = {}
    for dt in (torch.float32, torch.float64):
        n_, a_ = N.detach().cpu().to(dt).clone(), z_avg.detach().cpu().to(dt).clone()
        k_ = None if k_rand is None else k_rand.detach().cpu().to(dt)
        emb, usage = ema_statements(n_, a_, n_total.detach().cpu().to(dt), encode_sum.detach().cpu().to(dt), k_, restart_thres, no_random_restart)
        out[dt] = (n_, a_, emb, usage)
    return out


def gate_of(ref):
    """the gate of DESIGN.md §9f for each of N, z_avg, embeddings: 8 x the largest deviation of the fp32 statements from float64"""
    f32, f64 = ref[torch.float32], ref[torch.float64]
    return [8.0 * float((f32[i].double() - f64[i]).abs().max()) for i in range(3)]
