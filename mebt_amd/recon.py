"""First-stage validation: how good is a 3D-VQGAN checkpoint on a data set.

The reference answers this in `VQGAN.validation_step` (mebt/vqgan.py:190-196): `val/recon_loss` = `F.l1_loss(x_recon, x) * l1_weight`,
`val/commitment_loss` = `0.25 * F.mse_loss(z, embeddings)` and `val/perplexity` = `exp(-sum p log(p + 1e-10))` of the batch's code
histogram (modules/codebook.py:64,93-94).  The literature adds the reconstruction's PSNR, SSIM and rFVD.  Everything but the FVD is a
sum over tensors that already sit in HBM, so three HIP operators (csrc/recon/recon.hip) take them there and only scalars are read back:

  abs_diff_sum      sum |x - y| per clip, fp64                                              -> recon_loss
  code_stats        code histogram (int64, accumulates over calls) and sum |z - e_id|^2      -> perplexity, codes used, commitment_loss
  clip_quality_u8   per frame of two uint8 clips: sum (a - b)^2 (exact) and the mean SSIM    -> PSNR, SSIM

SSIM is Wang et al.'s: an 11 x 11 Gaussian window of sigma 1.5, valid positions only, per channel on the byte values,
C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, the mean over positions and channels.  All three operators are bitwise reproducible (fixed-order
fp64 partials, no float atomics).  The `*_twin` functions are the float64 torch statements of the same definitions: what the tests hold
the kernels to, and what reproduces the reference's figures on the CPU oracle; the product never calls them.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

ABS_CHUNK = 16384                 # MEBT_RECON_ABS_CHUNK
TILE_H, TILE_W = 16, 32           # MEBT_RECON_TILE_H / _W
CODE_ROWS = 16                    # MEBT_RECON_CODE_ROWS
WIN, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
FIELDS = ["recon_loss", "commitment_loss", "perplexity", "perplexity_set", "codes_used", "PSNR", "SSIM", "identical_frames", "n_clips"]


def ssim_window():
    """the 11 taps g_i = exp(-(i - 5)^2 / (2 sigma^2)), normalised in float64"""
    g = np.exp(-((np.arange(WIN, dtype=np.float64) - WIN // 2) ** 2) / (2 * SIGMA * SIGMA))
    return g / g.sum()


def _cdiv(a, b):
    return -(-a // b)


def _need(who, t, dtype, ndim=None):
    if not torch.is_tensor(t) or t.dtype != dtype or (ndim is not None and t.dim() != ndim):
        raise ValueError(f"{who}: expected {str(dtype).split('.')[-1]}{'' if ndim is None else f' of {ndim} dims'}, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if not t.is_cuda:
        raise ValueError(f"{who} runs on the GPU: move the tensors to the device first")
    return t.contiguous()


# ---- device side -----------------------------------------------------------------------------------------------------------------
def abs_diff_sum(x, y):
    """x, y float32 [B, ...] on the GPU -> float64 [B]: sum |x - y| per clip"""
    x, y = _need("abs_diff_sum", x, torch.float32), _need("abs_diff_sum", y, torch.float32)
    if x.shape != y.shape or x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"abs_diff_sum: shapes {tuple(x.shape)} and {tuple(y.shape)}")
    B = int(x.shape[0])
    n = x.numel() // B
    out = torch.empty(B, device=x.device, dtype=torch.float64)
    nbytes = 8 * B * _cdiv(n, ABS_CHUNK)
    scratch = _lib.scratch(nbytes, x.device)
    _lib.check(_lib.load().mebt_op_abs_diff_sum(_lib.ptr(x), _lib.ptr(y), _lib.ptr(out), B, n, _lib.ptr(scratch), nbytes, _lib.cur_stream()))
    return out


def clip_quality_u8(a, b):
    """a, b uint8 [..., H, W, 3] on the GPU (frames [N, H, W, 3] or clips [B, T, H, W, 3]) -> (sq_err int64 [...], ssim float64 [...])
    per frame: the exact sum of squared byte differences and the mean SSIM"""
    a, b = _need("clip_quality_u8", a, torch.uint8), _need("clip_quality_u8", b, torch.uint8)
    if a.shape != b.shape or a.dim() < 4 or a.shape[-1] != 3 or a.numel() == 0:
        raise ValueError(f"clip_quality_u8: expected two uint8 [..., H, W, 3] of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    lead, (H, W) = tuple(a.shape[:-3]), (int(a.shape[-3]), int(a.shape[-2]))
    N = a.numel() // (H * W * 3)
    sq = torch.empty(N, device=a.device, dtype=torch.int64)
    ssim = torch.empty(N, device=a.device, dtype=torch.float64)
    nbytes = 16 * N * _cdiv(max(H - 10, 1), TILE_H) * _cdiv(max(W - 10, 1), TILE_W)
    scratch = _lib.scratch(nbytes, a.device)
    _lib.check(_lib.load().mebt_op_clip_quality_u8(_lib.ptr(a), _lib.ptr(b), _lib.ptr(sq), _lib.ptr(ssim), N, H, W, _lib.ptr(scratch), nbytes,
                                                   _lib.cur_stream()))
    return sq.view(lead), ssim.view(lead)


def code_stats(ids, z, embeddings, hist=None):
    """ids int64 [...] (M of them), z float32 [M, d] or [..., d], embeddings float32 [n_codes, d], on the GPU -> (hist int64 [n_codes],
    sq_sum float64 [1]).  `hist` given: the counts are ADDED to it (a data set accumulates); None: a zeroed one is made.  Ids outside
    [0, n_codes) are skipped for both."""
    ids = _need("code_stats", ids, torch.int64).view(-1)
    emb = _need("code_stats", embeddings, torch.float32, 2)
    n_codes, d = int(emb.shape[0]), int(emb.shape[1])
    z = _need("code_stats", z, torch.float32)
    M = ids.numel()
    if M == 0 or z.numel() != M * d:
        raise ValueError(f"code_stats: {M} ids, z {tuple(z.shape)}, embeddings {tuple(emb.shape)}")
    if hist is None:
        hist = torch.zeros(n_codes, device=ids.device, dtype=torch.int64)
    elif (not torch.is_tensor(hist) or hist.dtype != torch.int64 or tuple(hist.shape) != (n_codes,) or hist.device != ids.device
          or not hist.is_contiguous()):
        raise ValueError(f"code_stats: `hist` must be contiguous int64 [{n_codes}] on {ids.device}")
    sq = torch.empty(1, device=ids.device, dtype=torch.float64)
    nbytes = 8 * _cdiv(M, CODE_ROWS)
    scratch = _lib.scratch(nbytes, ids.device)
    _lib.check(_lib.load().mebt_op_code_stats(_lib.ptr(ids), _lib.ptr(z), _lib.ptr(emb), _lib.ptr(hist), _lib.ptr(sq), M, n_codes, d,
                                              _lib.ptr(scratch), nbytes, _lib.cur_stream()))
    return hist, sq


# ---- the definitions in float64 torch (any device) ---------------------------------------------------------------------------------
def abs_diff_sum_twin(x, y):
    B = x.shape[0]
    return (x.double().reshape(B, -1) - y.double().reshape(B, -1)).abs().sum(1)


def ssim_map_twin(a, b):
    """uint8 [N, H, W, 3] x 2 -> the float64 SSIM map [N, 3, H - 10, W - 10]"""
    g = torch.from_numpy(ssim_window()).to(a.device)
    w = (g[:, None] * g[None, :])[None, None]

    def blur(t):
        n, c, h, ww = t.shape
        return F.conv2d(t.reshape(n * c, 1, h, ww), w).reshape(n, c, h - WIN + 1, ww - WIN + 1)

    u = a.double().permute(0, 3, 1, 2) - 128.0                  # centred: the variances are shift invariant
    v = b.double().permute(0, 3, 1, 2) - 128.0
    mu, mv = blur(u), blur(v)
    var_a, var_b, cov = blur(u * u) - mu * mu, blur(v * v) - mv * mv, blur(u * v) - mu * mv
    ma, mb = mu + 128.0, mv + 128.0
    return ((2 * ma * mb + C1) * (2 * cov + C2)) / ((ma * ma + mb * mb + C1) * (var_a + var_b + C2))


def clip_quality_u8_twin(a, b):
    lead, (H, W) = tuple(a.shape[:-3]), (int(a.shape[-3]), int(a.shape[-2]))
    if H < WIN or W < WIN:
        raise ValueError(f"clip_quality_u8_twin: the {WIN} x {WIN} window needs H, W >= {WIN}, got {H} x {W}")
    a, b = a.reshape(-1, H, W, 3), b.reshape(-1, H, W, 3)
    d = a.to(torch.int64) - b.to(torch.int64)
    return (d * d).sum((1, 2, 3)).view(lead), ssim_map_twin(a, b).mean((1, 2, 3)).view(lead)


def code_stats_twin(ids, z, embeddings, hist=None):
    ids = ids.reshape(-1)
    n_codes, d = embeddings.shape
    ok = (ids >= 0) & (ids < n_codes)
    kept = ids[ok]
    h = torch.bincount(kept, minlength=n_codes)
    diff = z.reshape(-1, d)[ok].double() - embeddings.double()[kept]
    return (h if hist is None else hist + h), (diff * diff).sum().reshape(1)


# ---- figures from the sums -------------------------------------------------------------------------------------------------------
def perplexity_of(hist):
    """exp(-sum p log(p + 1e-10)), p = hist / sum(hist) (codebook.py:93-94), float64, on the histogram's device"""
    h = hist.double()
    p = h / h.sum()
    return torch.exp(-(p * torch.log(p + 1e-10)).sum())


def psnr_of(sq_err, pixels):
    """10 log10(255^2 / MSE) per frame from the squared-error sums over `pixels` bytes; 0 where the frames are identical (see
    ReconAccumulator: those are counted apart)"""
    mse = sq_err.double() / pixels
    return torch.where(sq_err > 0, 10.0 * torch.log10(255.0 ** 2 / mse.clamp_min(1e-300)), torch.zeros_like(mse))


class ReconAccumulator:
    """adds up the dicts of `VQGAN.reconstruct_stats` on the device; `result()` reads everything once.

    recon_loss / commitment_loss: the reference's figures over the whole set (equal to its per-batch values averaged with the batch
    sizes as weights); perplexity: the same average of the per-batch perplexities, which is what the reference logs; perplexity_set:
    the perplexity of the whole set's histogram; codes_used: the fraction of codes hit at least once; PSNR: the mean over frames
    of 10 log10(255^2 / MSE), frames without any error left out and counted as identical_frames; SSIM: the mean over frames.  When the
    dicts carry `lpips` (reconstruct_stats(lpips_every=k)), `result()` ends with LPIPS: the mean over all scored frames."""

    def __init__(self, n_codes, l1_weight=4.0, device="cuda"):
        self.l1_weight = float(l1_weight)
        self.hist = torch.zeros(n_codes, device=device, dtype=torch.int64)
        self.sums = torch.zeros(6, device=device, dtype=torch.float64)    # |x - y|, |z - e|^2, B * perplexity, PSNR, SSIM, identical frames
        self.lpips_sum = torch.zeros((), device=device, dtype=torch.float64)
        self.n_clips = self.n_values = self.n_z = self.n_frames = self.n_lpips = 0

    def add(self, st):
        B = int(st["abs_sum"].shape[0])
        psnr = psnr_of(st["sq_err"], st["frame_bytes"])
        self.hist += st["hist"]
        self.sums += torch.stack([st["abs_sum"].sum(), st["commit_sq_sum"].sum(), B * perplexity_of(st["hist"]), psnr.sum(),
                                  st["ssim"].sum(), (st["sq_err"] == 0).sum().double()])
        self.n_clips += B
        self.n_values += st["recon"].numel()
        self.n_z += st["z_values"]
        self.n_frames += st["sq_err"].numel()
        if st.get("lpips") is not None:
            self.lpips_sum += st["lpips"].double().sum()
            self.n_lpips += st["lpips"].numel()

    def result(self):
        if self.n_clips == 0:
            raise ValueError("ReconAccumulator: no batch was added")
        s = self.sums.cpu().tolist()
        hist = self.hist.cpu()
        identical = int(round(s[5]))
        differing = self.n_frames - identical
        res = {"recon_loss": s[0] / self.n_values * self.l1_weight, "commitment_loss": 0.25 * s[1] / self.n_z,
               "perplexity": s[2] / self.n_clips, "perplexity_set": float(perplexity_of(hist)),
               "codes_used": float((hist > 0).sum()) / hist.numel(),
               "PSNR": s[3] / differing if differing else math.inf, "SSIM": s[4] / self.n_frames,
               "identical_frames": identical, "n_clips": self.n_clips}
        if self.n_lpips:
            res["LPIPS"] = float(self.lpips_sum) / self.n_lpips
        return res
