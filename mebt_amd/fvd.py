"""FVD / KVD — the API of reference mebt/fvd/fvd.py on the HIP Inception-I3D (mebt_amd/i3d.py).

The embedding (I3D forward) is the hot path and runs on the GPU only; the statistics (`frechet_distance`, `polynomial_mmd`) run on
the host in float64 numpy, with the reference's formulas: the SVD matrix square root of tensorflow-gan including its
`where(s < eps, s, sqrt(s))`, and the degree-3 polynomial kernel with gamma = 1 / d, coef0 = 1 (sklearn's defaults).
Differences from the reference: `get_logits` takes any N (no `% MAX_BATCH` assert), `MAX_BATCH` (clips per forward) defaults to
32 and follows $MEBT_I3D_BATCH, `load_fvd_model` takes a checkpoint path, and non-finite fp16 logits raise.
"""
import os

import numpy as np
import torch

from .i3d import InceptionI3d, TARGET_RESOLUTION, preprocess_uint8  # noqa: F401

MAX_BATCH = int(os.environ.get("MEBT_I3D_BATCH", "32"))
FVD_SAMPLE_SIZE = 2048
DEFAULT_CKPT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mebt", "fvd", "i3d_pretrained_400.pt")


def _model_device(i3d):
    return i3d.logits.conv3d.weight.device


def preprocess(videos, target_resolution=TARGET_RESOLUTION, device="cuda"):
    """fvd.py:17-28: uint8 [B, T, H, W, C] (numpy or tensor) -> fp32 [B, C, T, *target_resolution] in [-1, 1], resized on the GPU"""
    if tuple(target_resolution) != tuple(TARGET_RESOLUTION):
        raise ValueError(f"the I3D preprocess kernel resizes to {TARGET_RESOLUTION}")
    v = videos if torch.is_tensor(videos) else torch.from_numpy(np.ascontiguousarray(videos))
    return preprocess_uint8(v.to(device), "f32").permute(0, 4, 1, 2, 3).contiguous()


def _check_finite(logits, i3d):
    if not torch.isfinite(logits).all():
        raise FloatingPointError(f"I3D produced non-finite logits in compute_dtype={i3d.compute_dtype!r}; "
                                 "rerun with the fp32 path (--i3d_dtype f32 / i3d.compute_dtype = 'f32')")
    return logits


def get_fvd_logits(videos, i3d, device, batch=None):
    """fvd.py:30-33: uint8 videos [N, T, H, W, C] -> logits [N, 400] on `device`.  The resize runs on the GPU, fused in front of
    the network, `batch` (default MAX_BATCH) clips per forward."""
    batch = int(batch or MAX_BATCH)
    dev = _model_device(i3d)
    out = []
    n = len(videos)
    with torch.no_grad():
        for i in range(0, n, batch):
            v = videos[i:i + batch]
            v = (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).to(dev)
            out.append(_check_finite(i3d.forward_uint8(v), i3d))
    logits = torch.cat(out, 0) if out else torch.empty(0, i3d._num_classes, device=dev)
    return logits.to(device) if device is not None else logits


def get_logits(i3d, videos, device, batch=None):
    """fvd.py:116-124 without the `% MAX_BATCH` assert: preprocessed videos [N, 3, T, 224, 224] -> logits [N, 400]"""
    batch = int(batch or MAX_BATCH)
    out = []
    with torch.no_grad():
        for i in range(0, videos.shape[0], batch):
            out.append(_check_finite(i3d(videos[i:i + batch].to(_model_device(i3d))), i3d))
    return torch.cat(out, 0).to(device)


def load_fvd_model(device, path=None, compute_dtype="f16"):
    """fvd.py:35-42 with a checkpoint search: `path`, then $MEBT_I3D_CKPT, then mebt/fvd/i3d_pretrained_400.pt (where the
    reference looks).  The checkpoint is a plain state_dict of the reference's InceptionI3d(400, in_channels=3)."""
    cands = [("path argument", path), ("$MEBT_I3D_CKPT", os.environ.get("MEBT_I3D_CKPT")), ("default", DEFAULT_CKPT)]
    chosen = next((p for _, p in cands if p and os.path.isfile(p)), None)
    if chosen is None:
        tried = "; ".join(f"{what}: {p or '(unset)'}" for what, p in cands)
        raise FileNotFoundError("no I3D checkpoint found (the Kinetics-400 `i3d_pretrained_400.pt` state_dict of the reference). "
                                f"Tried, in order: {tried}")
    i3d = InceptionI3d(400, in_channels=3)
    i3d.load_state_dict(torch.load(chosen, map_location="cpu", weights_only=True), strict=True)
    i3d = i3d.to(device)
    i3d.eval()
    i3d.compute_dtype = compute_dtype
    return i3d


def _np64(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=np.float64).reshape(len(x), -1)


def _symmetric_matrix_square_root(mat, eps=1e-10):
    """tensorflow-gan classifier_metrics.py:161 as in fvd.py:46-49: u diag(s or sqrt(s)) v^T of the SVD"""
    u, s, vh = np.linalg.svd(mat)
    si = np.where(s < eps, s, np.sqrt(s))
    return (u * si) @ vh


def trace_sqrt_product(sigma, sigma_v):
    sqrt_sigma = _symmetric_matrix_square_root(sigma)
    return np.trace(_symmetric_matrix_square_root(sqrt_sigma @ (sigma_v @ sqrt_sigma)))


def cov(m):
    """unbiased covariance of the rows' features (fvd.py:58-89, rowvar=False)"""
    mc = m - m.mean(axis=0, keepdims=True)
    return mc.T @ mc / (m.shape[0] - 1)


def frechet_distance(x1, x2):
    """fvd.py:92-103 in float64: |m1 - m2|^2 + tr(S1 + S2) - 2 tr sqrt(S1^1/2 S2 S1^1/2)"""
    x1, x2 = _np64(x1), _np64(x2)
    s1, s2 = cov(x1), cov(x2)
    trace = np.trace(s1 + s2) - 2.0 * trace_sqrt_product(s1, s2)
    return float(trace + np.sum((x1.mean(0) - x2.mean(0)) ** 2))


def polynomial_kernel(X, Y=None, degree=3, coef0=1.0):
    Y = X if Y is None else Y
    return (X @ Y.T / X.shape[1] + coef0) ** degree


def polynomial_mmd(X, Y):
    """fvd.py:106-119: unbiased MMD^2 with the degree-3 polynomial kernel"""
    X, Y = _np64(X), _np64(Y)
    m, n = X.shape[0], Y.shape[0]
    kxx, kyy, kxy = polynomial_kernel(X), polynomial_kernel(Y), polynomial_kernel(X, Y)
    kxx_sum = (kxx.sum() - np.diagonal(kxx).sum()) / (m * (m - 1))
    kyy_sum = (kyy.sum() - np.diagonal(kyy).sum()) / (n * (n - 1))
    return float(kxx_sum + kyy_sum - 2 * kxy.sum() / (m * n))


def compute_fvd(real, samples, i3d, device=torch.device('cuda')):
    """fvd.py:127-133: real, samples uint8 [N, T, H, W, C] -> FVD"""
    first = get_fvd_logits(real, i3d, device)
    second = get_fvd_logits(samples, i3d, device)
    return frechet_distance(first, second)
