"""VQGAN — host-side mirror of the inference path of reference mebt/vqgan.py (`VQGAN.encode`, `VQGAN.decode`, :82-93) on the HIP
operators of csrc/vqgan.hip.  Same constructor argument (`args` namespace with n_hiddens / downsample / image_channels /
embedding_dim / n_codes), module tree and state-dict names (`encoder.conv_first.conv.weight`, `encoder.conv_blocks.0.res.norm1.weight`,
`decoder.conv_blocks.0.up.convt.weight`, `pre_vq_conv.conv.weight`, `codebook.embeddings`, ...) so reference checkpoints load;
the discriminators are not built (their keys are ignored on load): of
first-stage training, `recon_backward` gives the gradients of recon_loss + commitment_loss + perceptual_loss (vqgan.py:98-116,183-184
before discriminator_iter_start) on the kernels of csrc/vqgan_bwd/vqgan_bwd.hip and csrc/lpips/lpips_bwd.hip, with the codebook frozen or, with
`update_codebook=True`, trained by the EMA update with random restarts of modules/codebook.py on csrc/codebook/codebook_train.hip;
`configure_optimizers` is the reference's autoencoder Adam and `train_step` one step of the two (python -m mebt_amd.train_vqgan); the `perceptual_model.*` tensors are kept for the LPIPS of mebt_amd/lpips.py (forward for validation, `value_and_grad` for the perceptual term).  `validation_step`
(vqgan.py:190-196) and `reconstruct_stats` report the reconstruction's quality through the metric operators of csrc/recon/recon.hip
(mebt_amd/recon.py) and, when the checkpoint carried the perceptual weights, csrc/lpips/lpips.hip.

The nn.Modules below only HOLD parameters (and, after `recon_backward`, their `.grad`); no autograd graph is ever built.  `encode` /
`decode` walk a launch plan: every convolution is one
`mebt_op_conv3d` call per output sub-lattice (1 for a convolution, 4 or 8 for a stride-2 transposed convolution), every
Normalize + SiLU one `mebt_op_groupnorm_silu`, the codebook search one `mebt_op_codebook_argmin`.  Activations stay
channels-last on the GPU; `compute_dtype` = "f16" (MFMA, BASELINE config 5) or "f32" (parity).  Weights are re-laid out
([Cout][tap][Cin]) and cast once, at the first call after a (re)load or after an in-place parameter update (the parameters' version
counters are part of the cache key, so an optimizer step is noticed).  No CPU / eager-torch compute path exists.
"""
import ctypes as C
import itertools
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import check, ptr, cur_stream


def _strides(downsample):
    n = np.array([int(math.log2(d)) for d in downsample])
    out = []
    for _ in range(int(n.max())):
        out.append(tuple(2 if d > 0 else 1 for d in n))                      # vqgan.py:277,320
        n = n - 1
    return out


class SamePadConv3d(nn.Module):
    """parameters of reference vqgan.py:374-398 (`conv` = nn.Conv3d, padding handled by the kernel's clamped gather)"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, bias=True, padding_type='replicate'):
        super().__init__()
        k = (kernel_size,) * 3 if isinstance(kernel_size, int) else tuple(kernel_size)
        s = (stride,) * 3 if isinstance(stride, int) else tuple(stride)
        if padding_type != 'replicate':
            raise NotImplementedError("only replicate padding (the reference default) is built")
        self.kernel_size, self.stride = k, s
        self.conv = nn.Conv3d(in_channels, out_channels, k, stride=s, padding=0, bias=bias)


class SamePadConvTranspose3d(nn.Module):
    """parameters of reference vqgan.py:401-424 (`convt` = nn.ConvTranspose3d)"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, bias=True, padding_type='replicate'):
        super().__init__()
        k = (kernel_size,) * 3 if isinstance(kernel_size, int) else tuple(kernel_size)
        s = (stride,) * 3 if isinstance(stride, int) else tuple(stride)
        self.kernel_size, self.stride = k, s
        self.convt = nn.ConvTranspose3d(in_channels, out_channels, k, stride=s, bias=bias, padding=tuple(kk - 1 for kk in k))


def Normalize(in_channels, norm_type='group'):
    if norm_type != 'group':
        raise NotImplementedError("only GroupNorm (norm_type='group', the reference default) is built")
    return nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)    # vqgan.py:258


class SiLU(nn.Module):                         # placeholder so that `final_block.0` keeps its index (vqgan.py:285-288)
    pass


class ResBlock(nn.Module):
    """parameters of reference vqgan.py:338-355 (in_channels == out_channels everywhere in Encoder / Decoder)"""

    def __init__(self, in_channels, out_channels=None, norm_type='group', padding_type='replicate'):
        super().__init__()
        out_channels = in_channels if out_channels is None else out_channels
        if in_channels != out_channels:
            raise NotImplementedError("ResBlock with a channel change (conv_shortcut) does not occur in the VQGAN")
        self.norm1 = Normalize(in_channels, norm_type)
        self.conv1 = SamePadConv3d(in_channels, out_channels, kernel_size=3, padding_type=padding_type)
        self.norm2 = Normalize(in_channels, norm_type)
        self.conv2 = SamePadConv3d(out_channels, out_channels, kernel_size=3, padding_type=padding_type)


class Encoder(nn.Module):
    def __init__(self, n_hiddens, downsample, image_channel=3, norm_type='group', padding_type='replicate'):
        super().__init__()
        self.conv_blocks = nn.ModuleList()
        self.conv_first = SamePadConv3d(image_channel, n_hiddens, kernel_size=3, padding_type=padding_type)
        out_channels = n_hiddens
        for i, stride in enumerate(_strides(downsample)):
            block = nn.Module()
            in_channels, out_channels = n_hiddens * 2 ** i, n_hiddens * 2 ** (i + 1)
            block.down = SamePadConv3d(in_channels, out_channels, 4, stride=stride, padding_type=padding_type)
            block.res = ResBlock(out_channels, out_channels, norm_type=norm_type)
            self.conv_blocks.append(block)
        self.final_block = nn.Sequential(Normalize(out_channels, norm_type), SiLU())
        self.out_channels = out_channels


class Decoder(nn.Module):
    def __init__(self, n_hiddens, upsample, image_channel, norm_type='group'):
        super().__init__()
        strides = _strides(upsample)
        max_us = len(strides)
        in_channels = n_hiddens * 2 ** max_us
        self.final_block = nn.Sequential(Normalize(in_channels, norm_type), SiLU())
        self.conv_blocks = nn.ModuleList()
        out_channels = in_channels
        for i, us in enumerate(strides):
            block = nn.Module()
            in_channels = in_channels if i == 0 else n_hiddens * 2 ** (max_us - i + 1)
            out_channels = n_hiddens * 2 ** (max_us - i)
            block.up = SamePadConvTranspose3d(in_channels, out_channels, 4, stride=us)
            block.res1 = ResBlock(out_channels, out_channels, norm_type=norm_type)
            block.res2 = ResBlock(out_channels, out_channels, norm_type=norm_type)
            self.conv_blocks.append(block)
        self.conv_last = SamePadConv3d(out_channels, image_channel, kernel_size=3)


class Codebook(nn.Module):
    """buffers of reference modules/codebook.py:13-24.  `update` is the EMA update with random restarts of codebook.py:66-89 and
    `init_from` the data-dependent initialisation of codebook.py:34-46, both on the operators of csrc/codebook/codebook_train.hip and
    in place on the three buffers.  `_epoch` counts the in-place rewrites of `embeddings` (a kernel that writes through a raw pointer
    does not move the tensor's version counter): `VQGAN._prepare` keys on it.  Nothing here runs unless it is called: `VQGAN.encode`
    never initialises or updates (in the reference, `forward` in training mode does both)."""

    def __init__(self, n_codes, embedding_dim, no_random_restart=False, restart_thres=1.0):
        super().__init__()
        self.register_buffer('embeddings', torch.randn(n_codes, embedding_dim))
        self.register_buffer('N', torch.zeros(n_codes))
        self.register_buffer('z_avg', self.embeddings.data.clone())
        self.n_codes, self.embedding_dim = n_codes, embedding_dim
        self._need_init = True
        self.no_random_restart = no_random_restart
        self.restart_thres = restart_thres
        self._epoch = 0

    def _rows(self, who, z):
        if not torch.is_tensor(z) or z.dtype != torch.float32 or not z.is_cuda or z.numel() == 0 or z.shape[-1] != self.embedding_dim:
            raise ValueError(f"Codebook.{who}: z must be float32 [..., {self.embedding_dim}] (channels-last) on the GPU, got "
                             f"{getattr(z, 'dtype', type(z))} {tuple(getattr(z, 'shape', ()))}")
        for name in ("embeddings", "N", "z_avg"):
            b = getattr(self, name)
            if b.dtype != torch.float32 or b.device != z.device or not b.is_contiguous():
                raise ValueError(f"Codebook.{who}: buffer `{name}` must be contiguous float32 on {z.device}")
        return z.contiguous().view(-1, self.embedding_dim)

    def restart_rows(self, z, restart_src=None, restart_noise=None, generator=None):
        """`_k_rand` of codebook.py:41,82-83: n_codes rows of the tiled, noised and permuted z.  z fp32 [M, d].  With R = ceil(n_codes / M)
        copies of z when M < n_codes (else 1), row j is z[src[j] mod M] + noise[j] * 0.01 / sqrt(d), the noise only when M < n_codes
        (`_tile`).  restart_src int64 [n_codes] with values in [0, R M) and restart_noise fp32 [n_codes, d] inject the draws (the parity
        tests: src = the reference's randperm[:n_codes], noise = the rows of its randn_like at those positions); None: drawn here on
        the device with `generator`."""
        z = self._rows("restart_rows", z)
        M, dev = z.shape[0], z.device
        tiled = M < self.n_codes
        R = -(-self.n_codes // M) if tiled else 1
        if restart_src is None:
            restart_src = torch.randperm(R * M, device=dev, generator=generator)[:self.n_codes]
        src = restart_src.to(dev, torch.int64).contiguous()
        if tuple(src.shape) != (self.n_codes,):
            raise ValueError(f"Codebook.restart_rows: restart_src must hold {self.n_codes} row numbers, got {tuple(src.shape)}")
        noise = None
        if tiled:
            if restart_noise is None:
                restart_noise = torch.randn(self.n_codes, self.embedding_dim, device=dev, dtype=torch.float32, generator=generator)
            noise = restart_noise.to(dev, torch.float32).contiguous()
            if tuple(noise.shape) != (self.n_codes, self.embedding_dim):
                raise ValueError(f"Codebook.restart_rows: restart_noise must be [{self.n_codes}, {self.embedding_dim}], got {tuple(noise.shape)}")
        out = torch.empty(self.n_codes, self.embedding_dim, device=dev, dtype=torch.float32)
        check(_lib.load().mebt_op_codebook_restart_rows(ptr(z), ptr(src), ptr(noise), ptr(out), M, self.n_codes, self.embedding_dim, cur_stream()))
        return out

    @torch.no_grad()
    def init_from(self, z, restart_src=None, restart_noise=None, generator=None):
        """codebook.py:34-46: embeddings = z_avg = restart rows of z, N = 1; clears `_need_init`"""
        k_rand = self.restart_rows(z, restart_src, restart_noise, generator)
        self.embeddings.copy_(k_rand)
        self.z_avg.copy_(k_rand)
        self.N.fill_(1.0)
        self._need_init = False
        self._epoch += 1

    @staticmethod
    def code_sums(ids, z, n_codes):
        """ids int64 [M], z fp32 [M, d] on the GPU -> (n_total fp32 [n_codes], encode_sum fp32 [n_codes, d]): codebook.py:68-69"""
        M, d = z.shape
        lib = _lib.load()
        n_total = torch.empty(n_codes, device=z.device, dtype=torch.float32)
        encode_sum = torch.empty(n_codes, d, device=z.device, dtype=torch.float32)
        nbytes = int(lib.mebt_codebook_sums_scratch_bytes(M, n_codes))
        scratch = _lib.scratch(nbytes, z.device)
        check(lib.mebt_op_codebook_sums(ptr(ids), ptr(z), ptr(n_total), ptr(encode_sum), M, n_codes, d, ptr(scratch), nbytes, cur_stream()))
        return n_total, encode_sum

    @torch.no_grad()
    def update(self, z, ids, restart_src=None, restart_noise=None, generator=None):
        """The EMA update of codebook.py:66-89 for one batch: z fp32 [..., d] channels-last (what the search read), ids int64, one per
        row.  -> the number of codes restarted (0-dim int32 on the device; 0 with `no_random_restart`).  The draws: `restart_rows`."""
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError("Codebook.update on several ranks needs the all-reduces of n_total and encode_sum and the broadcast of "
                                      "the restart rows (codebook.py:70-72,84-85): data-parallel first-stage training is not built")
        z = self._rows("update", z)
        ids = ids.reshape(-1).contiguous()
        if ids.dtype != torch.int64 or ids.device != z.device or ids.numel() != z.shape[0]:
            raise ValueError(f"Codebook.update: {z.shape[0]} rows of z need as many int64 ids on {z.device}, got {ids.dtype} {tuple(ids.shape)}")
        lib = _lib.load()
        n_total, encode_sum = self.code_sums(ids, z, self.n_codes)
        k_rand = None if self.no_random_restart else self.restart_rows(z, restart_src, restart_noise, generator)
        restarted = torch.empty(1, device=z.device, dtype=torch.int32)
        nbytes = int(lib.mebt_codebook_ema_scratch_bytes(self.n_codes))
        scratch = _lib.scratch(nbytes, z.device)
        check(lib.mebt_op_codebook_ema(ptr(self.N), ptr(self.z_avg), ptr(self.embeddings), ptr(n_total), ptr(encode_sum), ptr(k_rand),
                                       ptr(restarted), self.n_codes, self.embedding_dim, float(self.restart_thres), ptr(scratch), nbytes,
                                       cur_stream()))
        self._epoch += 1
        return restarted[0]

    def dictionary_lookup(self, encodings):
        """codebook.py:99-101 -> [..., embedding_dim] fp32"""
        ids = encodings.reshape(-1).contiguous()
        out = torch.empty(ids.numel(), self.embedding_dim, device=ids.device, dtype=torch.float32)
        check(_lib.load().mebt_op_embedding_rows(_lib.F32, ptr(ids), ptr(self.embeddings), ptr(out), ids.numel(), self.embedding_dim,
                                                 self.n_codes, cur_stream()))
        return out.view(*encodings.shape, self.embedding_dim)


class _Conv:
    """one prepared convolution: re-laid-out weights of every output sub-lattice + the integer geometry"""

    def __init__(self, weight, bias, kernel, stride, transposed, dtype):
        dev = weight.device
        tdt = torch.float16 if dtype == "f16" else torch.float32
        self.bias = bias.detach().to(dev, torch.float32).contiguous() if bias is not None else None
        self.transposed, self.kernel, self.stride = transposed, kernel, stride
        self.classes = []            # (pi, taps [n,3] int, weights [Cout, n, Cin])
        self.sels = []               # transposed: per class, the (kt, kh, kw) of its taps in the nn.ConvTranspose3d weight
        self._plans = {}             # input dims -> data-gradient plan
        w = weight.detach().to(torch.float32)
        if not transposed:
            self.cout, self.cin = w.shape[0], w.shape[1]
            pad_front = [(k - s) // 2 + (k - s) % 2 for k, s in zip(kernel, stride)]                     # vqgan.py:385-388
            taps = [(kt - pad_front[0], kh - pad_front[1], kw - pad_front[2]) for kt in range(kernel[0]) for kh in range(kernel[1])
                    for kw in range(kernel[2])]
            wr = w.permute(0, 2, 3, 4, 1).reshape(self.cout, len(taps), self.cin)                       # [Cout][tap][Cin]
            self.classes.append(((0, 0, 0), taps, wr.to(tdt).contiguous()))
            self.os, self.sm = (1, 1, 1), stride
        else:
            self.cin, self.cout = w.shape[0], w.shape[1]
            # out o = i_p * s - (k - 1) + kk over the replicate-padded input i_p (pad front = (k-s)//2 + (k-s)%2); per dimension
            # and output parity pi (stride 2) only kk == (pi + k - 1) mod 2 contribute: i = o' + (pi + k - 1 - kk) / 2 - pad_front
            per_dim = []
            for k, s in zip(kernel, stride):
                pf = (k - s) // 2 + (k - s) % 2
                cls = {}
                for pi in range(s):
                    lst = []
                    for kk in range(k):
                        num = pi + (k - 1) - kk
                        if num % s == 0:
                            lst.append((kk, num // s - pf))
                    cls[pi] = lst
                per_dim.append(cls)
            for pt in range(stride[0]):
                for ph in range(stride[1]):
                    for pw in range(stride[2]):
                        taps, sel = [], []
                        for kt, ot in per_dim[0][pt]:
                            for kh, oh in per_dim[1][ph]:
                                for kw, ow in per_dim[2][pw]:
                                    taps.append((ot, oh, ow))
                                    sel.append((kt, kh, kw))
                        idx = torch.tensor(sel, device=dev)
                        wc = w[:, :, idx[:, 0], idx[:, 1], idx[:, 2]]                                    # [Cin, Cout, n]
                        self.classes.append(((pt, ph, pw), taps, wc.permute(1, 2, 0).to(tdt).contiguous()))
                        self.sels.append(sel)
            self.os, self.sm = stride, (1, 1, 1)

    def out_dims(self, dims):
        if self.transposed:
            return tuple(d * s for d, s in zip(dims, self.stride))
        return tuple(d // s for d, s in zip(dims, self.stride))

    # ---- backward geometry (host side only: integers and weight re-layouts) -------------------------------------------------------
    def class_counts(self, od, pi):
        return [(o - p + s - 1) // s for o, p, s in zip(od, pi, self.os)]

    def dgrad_plan(self, dims):
        """The data gradient of this layer at input size `dims`, as convolutions of dy on the PADDED input lattice.  The forward reads,
        for output voxel o = o' * os + pi and tap j, the input position p = o' * sm + tap[j] before the clamp; the lattice holds every such
        p, q = p - lo per dimension (`front` = -lo, size `pd`).  dxp[q] = sum w[co][j][ci] dy[o] over the (o', j) with o' * sm + tap[j] == p,
        dy read as ZERO outside its box: the caller copies dy into a zero box of size `zd` at offset `fz`, wide enough that no tap
        leaves it.  A convolution (os = 1) gives one class per parity of q modulo sm (a transposed convolution of dy); a transposed
        one (sm = 1) gives a single strided class over the taps of all its forward classes.  `classes`: dicts os / pi / sm / cq (class
        counts) / taps (into the zero box) / w ([Cin][n][Cout], None for a parity no tap reaches)."""
        key = tuple(dims)
        if key in self._plans:
            return self._plans[key]
        od = self.out_dims(dims)
        taps_all = [t for _, taps, _ in self.classes for t in taps]
        lo = [min(0, min(t[k] for t in taps_all)) for k in range(3)]
        hi = [max(0, max(t[k] for t in taps_all)) for k in range(3)]
        cmax = [max(self.class_counts(od, pi)[k] for pi, _, _ in self.classes) for k in range(3)]
        pd = [max((cmax[k] - 1) * self.sm[k] + hi[k], dims[k] - 1) - lo[k] + 1 for k in range(3)]
        gcls = []
        if not self.transposed:
            (_, taps, w), = self.classes
            for r in itertools.product(*[range(s) for s in self.sm]):
                sel, offs = [], []
                for j, t in enumerate(taps):
                    num = [r[k] + lo[k] - t[k] for k in range(3)]
                    if all(n % s == 0 for n, s in zip(num, self.sm)):
                        sel.append(j)
                        offs.append(tuple(n // s for n, s in zip(num, self.sm)))
                cq = [(pd[k] - r[k] + self.sm[k] - 1) // self.sm[k] for k in range(3)]
                gcls.append(dict(os=tuple(self.sm), pi=r, sm=(1, 1, 1), cq=cq, offs=offs,
                                 w=w[:, sel, :].permute(2, 1, 0).contiguous() if sel else None))
        else:
            offs, ws = [], []
            for pi, taps, w in self.classes:
                offs += [tuple((lo[k] - t[k]) * self.os[k] + pi[k] for k in range(3)) for t in taps]
                ws.append(w)
            gcls.append(dict(os=(1, 1, 1), pi=(0, 0, 0), sm=tuple(self.os), cq=list(pd), offs=offs,
                             w=torch.cat(ws, dim=1).permute(2, 1, 0).contiguous()))
        live = [c for c in gcls if c["offs"] and min(c["cq"]) > 0]
        mn = [min([0] + [min(o[k] for o in c["offs"]) for c in live]) for k in range(3)]
        mx = [max([od[k] - 1] + [(c["cq"][k] - 1) * c["sm"][k] + max(o[k] for o in c["offs"]) for c in live]) for k in range(3)]
        fz = [-mn[k] for k in range(3)]
        zd = [fz[k] + mx[k] + 1 for k in range(3)]
        for c in gcls:
            c["taps"] = [tuple(o[k] + fz[k] for k in range(3)) for o in c["offs"]]
            assert len(c["taps"]) <= 64 and all(-128 <= v < 128 for t in c["taps"] for v in t), (self.kernel, self.stride)
        plan = dict(front=[-v for v in lo], pd=pd, fz=fz, zd=zd, classes=gcls)
        self._plans[key] = plan
        return plan

    def full_weight_grad(self, dws):
        """per-class gradients [Cout][n][Cin] (fp32) -> the shape of the nn.Conv3d / nn.ConvTranspose3d weight"""
        if not self.transposed:
            return dws[0].view(self.cout, *self.kernel, self.cin).permute(0, 4, 1, 2, 3).contiguous()
        g = torch.zeros(self.cin, self.cout, *self.kernel, device=dws[0].device, dtype=torch.float32)
        for dw, sel in zip(dws, self.sels):
            idx = torch.tensor(sel, device=dw.device)
            g[:, :, idx[:, 0], idx[:, 1], idx[:, 2]] = dw.permute(2, 0, 1)
        return g


class _Desc(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("resid", C.c_void_p),
                ("B", C.c_int32), ("Ti", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32), ("Cin", C.c_int32),
                ("To", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("Cout", C.c_int32),
                ("cT", C.c_int32), ("cH", C.c_int32), ("cW", C.c_int32),
                ("os", C.c_int32 * 3), ("pi", C.c_int32 * 3), ("sm", C.c_int32 * 3), ("ntaps", C.c_int32),
                ("tap", (C.c_int8 * 4) * 64), ("in_mode", C.c_int32), ("out_mode", C.c_int32)]

    @classmethod
    def of(cls, x, out, w, B, idims, cin, odims, cout, counts, os_, pi, sm, taps, in_mode, out_mode, bias=None, resid=None):
        """one class of a convolution: tensors (or None) + the integer geometry of include/mebt_hip.h's mebt_conv3d_desc"""
        d = cls()
        d.in_, d.out, d.w, d.bias, d.resid = ptr(x), ptr(out), ptr(w), ptr(bias), ptr(resid)
        d.B, d.Ti, d.Hi, d.Wi, d.Cin = B, idims[0], idims[1], idims[2], cin
        d.To, d.Ho, d.Wo, d.Cout = odims[0], odims[1], odims[2], cout
        d.cT, d.cH, d.cW = counts
        for k in range(3):
            d.os[k], d.pi[k], d.sm[k] = os_[k], pi[k], sm[k]
        d.ntaps = len(taps)
        for j, t in enumerate(taps):
            d.tap[j][0], d.tap[j][1], d.tap[j][2] = t
        d.in_mode, d.out_mode = in_mode, out_mode
        return d


class VQGAN(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.embedding_dim, self.n_codes = args.embedding_dim, args.n_codes
        norm_type = getattr(args, "norm_type", "group")
        padding_type = getattr(args, "padding_type", "replicate")
        image_channels = getattr(args, "image_channels", 3)
        self.encoder = Encoder(args.n_hiddens, args.downsample, image_channels, norm_type, padding_type)
        self.decoder = Decoder(args.n_hiddens, args.downsample, image_channels, norm_type)
        self.enc_out_ch = self.encoder.out_channels
        self.pre_vq_conv = SamePadConv3d(self.enc_out_ch, args.embedding_dim, 1, padding_type=padding_type)
        self.post_vq_conv = SamePadConv3d(args.embedding_dim, self.enc_out_ch, 1)
        self.codebook = Codebook(args.n_codes, args.embedding_dim, no_random_restart=bool(getattr(args, "no_random_restart", False)),
                                 restart_thres=float(getattr(args, "restart_thres", 1.0)))
        self.compute_dtype = "f16"
        self.use_mfma = True
        self._prepared = None
        self._tape = None            # recon_backward's training forward: {layer -> what its backward reads}
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_prepared", None))

    @property
    def latent_shape(self):
        a = self.args
        shape = (a.sequence_length // a.sample_every_n_frames, a.resolution, a.resolution)
        return tuple(s // d for s, d in zip(shape, a.downsample))

    @classmethod
    def load_from_checkpoint(cls, path, map_location="cpu"):
        """Lightning checkpoint of the reference (download.py:56-61): {'state_dict', 'hyper_parameters': {'args': Namespace}}"""
        ck = torch.load(path, map_location=map_location, weights_only=False)
        hp = ck.get("hyper_parameters", {})
        model = cls(hp["args"] if "args" in hp else hp)
        model.load_state_dict(ck["state_dict"], strict=False)
        return model

    def load_state_dict(self, state_dict, strict=True, **kw):
        """The discriminators of a reference checkpoint are not part of the inference path and are skipped.  Its `perceptual_model.*`
        tensors (the reference's LPIPS sub-module: 13 VGG-16 convolutions, five `lin` layers, two scaling buffers) are kept as CPU
        tensors in the plain attribute `lpips_weights`, not as parameters or buffers: `state_dict()` and `.to()` do not see them.
        A partial set raises, naming what is missing; a state dict without any leaves an earlier set in place."""
        from . import lpips as _lpips
        skip = ("image_discriminator.", "video_discriminator.", _lpips.PREFIX)
        sd = {k: v for k, v in state_dict.items() if not k.startswith(skip)}
        if any(k.startswith(_lpips.PREFIX) for k in state_dict):
            own = _lpips.extract({k: v for k, v in state_dict.items() if k.startswith(_lpips.PREFIX)})
            if own is not None:
                self.lpips_weights = own
        if "codebook.embeddings" in sd:
            self.codebook._need_init = False         # trained codes are kept on resume (the reference re-initialises them)
        return super().load_state_dict(sd, strict=strict, **kw)

    @property
    def lpips_weights(self):
        return self.__dict__.get("_lpips_weights")

    @lpips_weights.setter
    def lpips_weights(self, own):
        self.__dict__["_lpips_weights"] = own
        self.__dict__["_lpips_built"] = None

    @property
    def lpips(self):
        """None without perceptual weights; else `mebt_amd.lpips.LPIPS` on the model's device, built at first use.  Its compute dtype is
        `lpips_dtype` ("f16" / "f32"), or the model's `compute_dtype` while that is None."""
        own = self.lpips_weights
        if own is None:
            return None
        from .lpips import LPIPS
        key = (self.__dict__.get("lpips_dtype") or self.compute_dtype, self.codebook.embeddings.device)
        built = self.__dict__.get("_lpips_built")
        if built is None or built[0] != key:
            built = (key, LPIPS(own, dtype=key[0], device=key[1]))
            self.__dict__["_lpips_built"] = built
        return built[1]

    # ---- preparation ---------------------------------------------------------------------------------------------------
    def _prepare(self):
        dev = self.codebook.embeddings.device
        if dev.type != "cuda":
            raise RuntimeError("mebt_amd.vqgan runs on MI355X only: move the model to the GPU (there is no CPU path in the product)")
        # the parameters' version counters: an optimizer step (an in-place update) makes the re-laid-out weights stale
        key = (self.compute_dtype, dev, tuple(p._version for p in self.parameters()), self.codebook.embeddings._version)
        if self._prepared is not None and self._prepared["key"] == key:
            if self._prepared["emb_epoch"] != self.codebook._epoch:          # Codebook.update / init_from rewrote the codes in place
                self._prepared["emb"] = self.codebook.embeddings.detach().to(torch.float32).contiguous()
                self._prepared["emb_epoch"] = self.codebook._epoch
            return self._prepared
        dt = self.compute_dtype
        prep = {"key": key, "convs": {}}

        def conv(mod):
            if isinstance(mod, SamePadConv3d):
                return _Conv(mod.conv.weight, mod.conv.bias, mod.kernel_size, mod.stride, False, dt)
            return _Conv(mod.convt.weight, mod.convt.bias, mod.kernel_size, mod.stride, True, dt)

        for name, mod in self.named_modules():
            if isinstance(mod, (SamePadConv3d, SamePadConvTranspose3d)):
                prep["convs"][name] = conv(mod)
        prep["emb"] = self.codebook.embeddings.detach().to(torch.float32).contiguous()
        prep["emb_epoch"] = self.codebook._epoch
        self._prepared = prep
        return prep

    # ---- launch helpers ----------------------------------------------------------------------------------------------------
    def _tdt(self):
        return _lib.torch_dtype(self.compute_dtype)

    def _code(self):
        return _lib.dtype_code(self.compute_dtype)

    def _conv(self, name, x, B, dims, resid=None, in_mode=0, out_mode=0):
        """x: channels-last [B, *dims, Cin] (or the fp32 video when in_mode = 1) -> (out, out_dims)"""
        cv = self._prepared["convs"][name]
        od = cv.out_dims(dims)
        dev = x.device
        if self._tape is not None:
            self._tape[name] = (x, dims, in_mode, out_mode)
        shape = (B, cv.cout, *od) if out_mode == 2 else (B, *od, cv.cout)         # mebt_conv3d_desc.out_mode
        out = torch.empty(shape, device=dev, dtype=self._tdt() if out_mode == 0 else torch.float32)
        lib = _lib.load()
        for pi, taps, w in cv.classes:
            d = _Desc.of(x, out, w, B, dims, cv.cin, od, cv.cout, cv.class_counts(od, pi), cv.os, pi, cv.sm, taps, in_mode, out_mode,
                         bias=cv.bias, resid=resid)
            check(lib.mebt_op_conv3d(self._code(), C.byref(d), 1 if self.use_mfma else 0, cur_stream()))
        return out, od

    def _norm_silu(self, gn, x, B, dims):
        Cc = x.shape[-1]
        y = torch.empty_like(x)
        stats = torch.empty(B * 64, device=x.device, dtype=torch.float32)
        g, b = gn.weight.detach().float().contiguous(), gn.bias.detach().float().contiguous()
        check(_lib.load().mebt_op_groupnorm_silu(self._code(), ptr(x), ptr(y), ptr(g), ptr(b), ptr(stats), B, int(np.prod(dims)), Cc,
                                                 cur_stream()))
        if self._tape is not None:
            self._tape[id(gn)] = (x, stats, B, dims)
        return y

    def _res(self, prefix, mod, x, B, dims):
        """ResBlock.forward (vqgan.py:357-370): x + conv2(silu(norm2(conv1(silu(norm1(x))))))"""
        h = self._norm_silu(mod.norm1, x, B, dims)
        h, _ = self._conv(prefix + ".conv1", h, B, dims)
        h = self._norm_silu(mod.norm2, h, B, dims)
        h, _ = self._conv(prefix + ".conv2", h, B, dims, resid=x)
        return h

    # ---- reference API ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode(self, x, include_embeddings=False):
        """VQGAN.encode (vqgan.py:82-88): x [B, C, T, H, W] float -> encodings [B, t, h, w] int64 (and, with include_embeddings,
        the quantised embeddings [B, c, t, h, w] first)"""
        z, B, dims = self._encode_z(x)
        ids = self._search(z).view(B, *dims)
        if include_embeddings:
            e = self.codebook.dictionary_lookup(ids)                                     # [B, t, h, w, c]
            return e.permute(0, 4, 1, 2, 3), ids                                         # a view: [B, c, t, h, w] (shift_dim, codebook.py:63)
        return ids

    def _encode_z(self, x):
        """pre_vq_conv(encoder(x)) -> (z fp32 [B, t, h, w, c], B, (t, h, w)); kept in `_last_z`"""
        self._prepare()
        x = x.to(torch.float32).contiguous()
        B, dims = x.shape[0], tuple(x.shape[2:])
        h, dims = self._conv("encoder.conv_first", x, B, dims, in_mode=1)
        for i, blk in enumerate(self.encoder.conv_blocks):
            h, dims = self._conv(f"encoder.conv_blocks.{i}.down", h, B, dims)
            h = self._res(f"encoder.conv_blocks.{i}.res", blk.res, h, B, dims)
        h = self._norm_silu(self.encoder.final_block[0], h, B, dims)
        z, dims = self._conv("pre_vq_conv", h, B, dims, out_mode=1)                    # fp32 [B, t, h, w, c] for the search
        self._last_z = z
        return z, B, dims

    def _search(self, z):
        """the arg-min of codebook.py:53-57 over the prepared codes -> ids int64 [M]"""
        M = z.numel() // self.embedding_dim
        emb = self._prepare()["emb"]
        esq = torch.empty(self.n_codes + 1, device=z.device, dtype=torch.float32)
        ids = torch.empty(M, device=z.device, dtype=torch.long)
        # large searches (config 5 at batch 16: 16384 x 16384 x 256): approximate scores on the bf16 MFMA GEMM + exact fp32 re-evaluation
        # of every code that can still be the arg-min (csrc/vqgan.hip codebook_filter_kernel); small ones: the exact fp32 GEMM directly
        if (self.use_mfma and self.embedding_dim % 64 == 0 and self.n_codes % 8 == 0 and M * self.n_codes >= (1 << 24)
                and os.environ.get("MEBT_CODEBOOK_FILTER", "1") != "0"):
            lowp = torch.empty((M + self.n_codes) * self.embedding_dim, device=z.device, dtype=torch.bfloat16)
            score = torch.empty(M, self.n_codes, device=z.device, dtype=torch.bfloat16)     # approximate scores: half the bytes of the exact path's matrix
            check(_lib.load().mebt_op_codebook_argmin_filtered(ptr(z), ptr(emb), ptr(score), ptr(esq), ptr(lowp), ptr(ids), M, self.n_codes,
                                                               self.embedding_dim, cur_stream()))
        else:
            score = torch.empty(M, self.n_codes, device=z.device, dtype=torch.float32)
            check(_lib.load().mebt_op_codebook_argmin(ptr(z), ptr(emb), ptr(score), ptr(esq), ptr(ids), M, self.n_codes, self.embedding_dim,
                                                      cur_stream()))
        return ids

    @torch.no_grad()
    def decode(self, encodings):
        """VQGAN.decode (vqgan.py:90-93): encodings [B, t, h, w] int64 -> video [B, C, T, H, W] fp32"""
        self._prepare()
        ids = encodings.contiguous()
        B, dims = ids.shape[0], tuple(ids.shape[1:])
        rows = ids.numel()
        h = torch.empty(B, *dims, self.embedding_dim, device=ids.device, dtype=self._tdt())
        check(_lib.load().mebt_op_embedding_rows(self._code(), ptr(ids), ptr(self._prepared["emb"]), ptr(h), rows, self.embedding_dim,
                                                 self.n_codes, cur_stream()))
        h, dims = self._conv("post_vq_conv", h, B, dims)
        h = self._norm_silu(self.decoder.final_block[0], h, B, dims)
        for i, blk in enumerate(self.decoder.conv_blocks):
            h, dims = self._conv(f"decoder.conv_blocks.{i}.up", h, B, dims)
            h = self._res(f"decoder.conv_blocks.{i}.res1", blk.res1, h, B, dims)
            h = self._res(f"decoder.conv_blocks.{i}.res2", blk.res2, h, B, dims)
        out, _ = self._conv("decoder.conv_last", h, B, dims, out_mode=2)
        return out

    def forward(self, x):
        """reconstruction (the inference part of vqgan.py:95-100): decode(encode(x))"""
        return self.decode(self.encode(x))

    # ---- backward of the reconstruction objective (vqgan.py:98-102,183-184 before discriminator_iter_start) on csrc/vqgan_bwd/vqgan_bwd.hip ----------
    def _acc(self, param, grad, flags):
        """autograd's accumulate semantics: `.grad` is created where it is None, else added to"""
        flags.append(torch.isfinite(grad).all())
        if param.grad is None:
            param.grad = grad.to(param.dtype).clone()
        else:
            param.grad.add_(grad.to(param.dtype))

    def _conv_wgrad(self, name, x, dy, B, dims, in_mode, dy_mode, inv_scale):
        """-> (weight gradient in the nn.Module's shape, bias gradient), fp32, the gradient scale removed"""
        cv = self._prepared["convs"][name]
        od = cv.out_dims(dims)
        lib = _lib.load()
        dws, db = [], None
        for pi, taps, _ in cv.classes:
            cls = cv.class_counts(od, pi)
            d = _Desc.of(x, dy, None, B, dims, cv.cin, od, cv.cout, cls, cv.os, pi, cv.sm, taps, in_mode, dy_mode)
            tiles = len(taps) * (-(-cv.cout // 64)) * (-(-cv.cin // 64))
            nsplit = max(1, min(256, -(-1024 // tiles), -(-B * int(np.prod(cls)) // 32)))
            nbytes = int(lib.mebt_conv3d_wgrad_scratch_bytes(C.byref(d), nsplit))
            scratch = _lib.scratch(nbytes, x.device)
            dw = torch.empty(cv.cout, len(taps), cv.cin, device=x.device, dtype=torch.float32)
            dbc = torch.empty(cv.cout, device=x.device, dtype=torch.float32)
            check(lib.mebt_op_conv3d_wgrad(self._code(), C.byref(d), ptr(dw), ptr(dbc), inv_scale, nsplit, ptr(scratch), nbytes, cur_stream()))
            dws.append(dw)
            db = dbc if db is None else db + dbc
        return cv.full_weight_grad(dws), db

    def _conv_dgrad(self, name, dy, B, dims, dy_mode=0, add=None, out_fp32=False):
        """dy (the layer's output gradient in the layout of its forward out_mode) -> dx channels-last [B, *dims, Cin] (+ add)"""
        cv = self._prepared["convs"][name]
        plan = cv.dgrad_plan(dims)
        od = cv.out_dims(dims)
        lib, dev = _lib.load(), dy.device
        fz, zd, pd, fr = plan["fz"], plan["zd"], plan["pd"], plan["front"]
        dyz = torch.empty(B, *zd, cv.cout, device=dev, dtype=self._tdt())
        check(lib.mebt_op_pad_zero(self._code(), ptr(dy), ptr(dyz), B, *od, *fz, *zd, cv.cout, dy_mode, cur_stream()))
        whole = all(c["w"] is not None for c in plan["classes"])
        dxp = (torch.empty if whole else torch.zeros)(B, *pd, cv.cin, device=dev, dtype=torch.float32)
        for c in plan["classes"]:
            if c["w"] is None or min(c["cq"]) <= 0:
                continue
            d = _Desc.of(dyz, dxp, c["w"], B, zd, cv.cout, pd, cv.cin, c["cq"], c["os"], c["pi"], c["sm"], c["taps"], 0, 1)
            check(lib.mebt_op_conv3d(self._code(), C.byref(d), 1 if self.use_mfma else 0, cur_stream()))
        dx = torch.empty(B, *dims, cv.cin, device=dev, dtype=torch.float32 if out_fp32 else self._tdt())
        check(lib.mebt_op_halo_fold(self._code(), ptr(dxp), ptr(add), ptr(dx), B, *dims, *pd, *fr, cv.cin, 1 if out_fp32 else 0, cur_stream()))
        return dx

    def _conv_bwd(self, name, dy, B, tape, inv_scale, flags, need_dx=True, add=None, out_fp32=False):
        x, dims, in_mode, out_mode = tape[name]
        mod = self.get_submodule(name)
        conv = mod.conv if isinstance(mod, SamePadConv3d) else mod.convt
        dw, db = self._conv_wgrad(name, x, dy, B, dims, in_mode, out_mode, inv_scale)
        self._acc(conv.weight, dw, flags)
        if conv.bias is not None:
            self._acc(conv.bias, db, flags)
        return self._conv_dgrad(name, dy, B, dims, out_mode, add, out_fp32) if need_dx else None

    def _norm_silu_bwd(self, gn, dy, tape, inv_scale, flags, add=None):
        x, stats, B, dims = tape[id(gn)]
        Cc, vox = x.shape[-1], int(np.prod(dims))
        lib = _lib.load()
        g, b = gn.weight.detach().float().contiguous(), gn.bias.detach().float().contiguous()
        dx = torch.empty_like(x)
        dg, dbt = torch.empty(Cc, device=x.device, dtype=torch.float32), torch.empty(Cc, device=x.device, dtype=torch.float32)
        nbytes = int(lib.mebt_groupnorm_silu_bwd_scratch_bytes(B, vox, Cc))
        scratch = _lib.scratch(nbytes, x.device)
        check(lib.mebt_op_groupnorm_silu_bwd(self._code(), ptr(x), ptr(stats), ptr(g), ptr(b), ptr(dy), ptr(add), ptr(dx), ptr(dg), ptr(dbt),
                                             inv_scale, B, vox, Cc, ptr(scratch), nbytes, cur_stream()))
        self._acc(gn.weight, dg, flags)
        self._acc(gn.bias, dbt, flags)
        return dx

    def _res_bwd(self, prefix, mod, g, B, tape, inv_scale, flags):
        """backward of x + conv2(silu(norm2(conv1(silu(norm1(x)))))): the skip's gradient is added where norm1's dx is stored"""
        h = self._conv_bwd(prefix + ".conv2", g, B, tape, inv_scale, flags)
        h = self._norm_silu_bwd(mod.norm2, h, tape, inv_scale, flags)
        h = self._conv_bwd(prefix + ".conv1", h, B, tape, inv_scale, flags)
        return self._norm_silu_bwd(mod.norm1, h, tape, inv_scale, flags, add=g)

    def default_grad_scale(self, n_video, n_z):
        """the power of two S that puts the L1 seed S * l1_weight / numel(x) into (2^-4, 2^-3]; with l1_weight 0, the
        quantiser seed's factor 0.5 / numel(z) instead"""
        c = float(self._hp("l1_weight", 4.0)) / n_video
        if c <= 0.0:
            c = 0.5 / n_z
        return 2.0 ** math.floor(math.log2(0.125 / c))

    def recon_backward(self, x, grad_scale=None, update_codebook=False, restart_src=None, restart_noise=None, init_src=None, init_noise=None,
                       generator=None, frame_idx=None):
        """The autoencoder objective of the reference before `discriminator_iter_start` (vqgan.py:98-116,183-184):
        loss = l1_weight * mean |x_recon - x| + 0.25 * mse(z, e.detach()) + perceptual_weight * mean_b LPIPS(x[b, :, idx_b],
        x_recon[b, :, idx_b]), the codebook frozen, the quantiser straight-through (codebook.py:64,91).  Runs the training forward (`encode` + `decode` recording every convolution's input, every GroupNorm's
        input and statistics, z and the ids), then the backward on the operators of csrc/vqgan_bwd/vqgan_bwd.hip, and ADDS the fp32 gradient to
        `.grad` of every parameter of encoder, decoder, pre_vq_conv and post_vq_conv (created where None: autograd's semantics, so
        `optimizer.zero_grad()` works as usual).  The backward is seeded with the power-of-two `grad_scale` S (None:
        `default_grad_scale`), removed exactly in the fp32 epilogues of the parameter-gradient kernels: in f16 mode the activation
        gradients are stored as fp16 and the unscaled seed l1_weight / numel(x) lies below fp16's range.
        -> {recon_loss, commitment_loss, perplexity (0-dim float64 on the device), encodings, grad_scale, finite, x_recon (the
        reconstruction the L1 seed's signs were taken from)}

        perceptual_weight > 0 needs the perceptual weights (`self.lpips`).  `frame_idx` (int [B]; None: drawn after the decode with
        `torch.randint(0, T, [B])`, as `validation_step` and vqgan.py:104 draw it) names the frame of every clip the term is taken on;
        `LPIPS.value_and_grad` adds S * perceptual_weight / B * dLPIPS/dx_recon into the L1 seed before `decoder.conv_last`'s backward
        (csrc/lpips/lpips_bwd.hip).  That branch runs at its own power-of-two scale, `self.perceptual_grad_scale` (None:
        `lpips.default_branch_scale`); an overflow in it clears `finite`.  The dict gains `perceptual_loss` (0-dim float64) and
        `frame_idx`.  With perceptual_weight 0 nothing is drawn and the dict is the one above.

        update_codebook (default False: the codebook stays frozen, as above) trains the codebook too, as the reference's forward does in
        training mode: while `codebook._need_init` is set, `Codebook.init_from(z)` runs after the encoder and before the arg-min
        (codebook.py:50-51), and `Codebook.update(z, ids)` runs after `mebt_op_vq_seed`, so that the commitment loss, the straight-through
        gradient and the decoder's input all use the codes from BEFORE the update (in the reference `F.embedding` has copied them by
        then).  The dict gains `codes_restarted` (0-dim int32 on the device).  restart_src / restart_noise and init_src / init_noise inject
        the draws of the update and of the initialisation (`Codebook.restart_rows`); `generator` seeds those drawn here."""
        pw = float(self._hp("perceptual_weight", 0.0))
        net = self.lpips if pw > 0.0 else None
        if pw > 0.0 and net is None:
            # a RuntimeError, as reconstruct_stats raises for the same lack; of the subclass the earlier refusal of this argument raised,
            # so that callers who caught that one still do
            raise NotImplementedError("recon_backward: perceptual_weight > 0 (the LPIPS backward) needs the perceptual weights (a checkpoint "
                                      "with perceptual_model.* tensors, or `lpips_weights` set from mebt_amd.lpips.read_file)")
        if update_codebook and torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError("recon_backward(update_codebook=True) on several ranks needs the all-reduces of n_total and encode_sum and "
                                      "the broadcast of the restart rows (codebook.py:70-72,84-85): data-parallel first-stage training is not built")
        from . import recon
        self._prepare()
        lib = _lib.load()
        x = x.to(torch.float32).contiguous()
        B = x.shape[0]
        self._tape = {}
        try:
            with torch.no_grad():
                z, _, dims = self._encode_z(x)
                if update_codebook and self.codebook._need_init:
                    self.codebook.init_from(z, init_src, init_noise, generator)
                ids = self._search(z).view(B, *dims)
            rec = self.decode(ids)
        finally:
            tape, self._tape = self._tape, None
        emb = self._prepared["emb"]
        hist, sq_sum = recon.code_stats(ids, z, emb)
        l1w = float(self._hp("l1_weight", 4.0))
        out = {"recon_loss": recon.abs_diff_sum(x.view(B, -1), rec.view(B, -1)).sum() / rec.numel() * l1w,
               "commitment_loss": 0.25 * sq_sum[0] / z.numel(), "perplexity": recon.perplexity_of(hist), "encodings": ids, "x_recon": rec}
        S = float(grad_scale) if grad_scale is not None else self.default_grad_scale(rec.numel(), z.numel())
        if not (S > 0.0 and math.isfinite(S) and math.frexp(S)[0] == 0.5):
            raise ValueError(f"recon_backward: grad_scale must be a positive power of two, got {grad_scale}")
        inv, flags = 1.0 / S, []
        with torch.no_grad():
            seed = torch.empty_like(rec)
            check(lib.mebt_op_l1_seed(ptr(rec), ptr(x), ptr(seed), rec.numel(), S * l1w / rec.numel(), cur_stream()))
            if net is not None:
                if frame_idx is None:
                    frame_idx = torch.randint(0, x.shape[2], [B])
                keep = bool(self.__dict__.get("_lpips_keep_tape"))          # tests only: the forward outputs the ReLU / pool decisions came from
                vals = net.value_and_grad(x, rec, frame_idx, seed, S * pw / B, grad_scale=self.__dict__.get("perceptual_grad_scale"),
                                          keep_tape=keep, flags=flags)
                if keep:
                    vals, out["lpips_tape"], _ = vals
                out["perceptual_loss"] = vals.mean() * pw
                out["frame_idx"] = torch.as_tensor(frame_idx).detach().to("cpu", torch.int64)
            g = self._conv_bwd("decoder.conv_last", seed, B, tape, inv, flags)
            for i in reversed(range(len(self.decoder.conv_blocks))):
                blk = self.decoder.conv_blocks[i]
                g = self._res_bwd(f"decoder.conv_blocks.{i}.res2", blk.res2, g, B, tape, inv, flags)
                g = self._res_bwd(f"decoder.conv_blocks.{i}.res1", blk.res1, g, B, tape, inv, flags)
                g = self._conv_bwd(f"decoder.conv_blocks.{i}.up", g, B, tape, inv, flags)
            g = self._norm_silu_bwd(self.decoder.final_block[0], g, tape, inv, flags)
            g_st = self._conv_bwd("post_vq_conv", g, B, tape, inv, flags, out_fp32=True)       # straight-through: lands on z
            dz = torch.empty_like(z)
            check(lib.mebt_op_vq_seed(ptr(z), ptr(emb), ptr(ids), ptr(g_st), ptr(dz), ids.numel(), self.embedding_dim, self.n_codes,
                                      S * 0.5 / z.numel(), cur_stream()))
            if update_codebook:                        # after the last reader of the old codes; nothing below reads the codebook
                out["codes_restarted"] = self.codebook.update(z, ids, restart_src, restart_noise, generator)
            g = self._conv_bwd("pre_vq_conv", dz, B, tape, inv, flags)
            g = self._norm_silu_bwd(self.encoder.final_block[0], g, tape, inv, flags)
            for i in reversed(range(len(self.encoder.conv_blocks))):
                g = self._res_bwd(f"encoder.conv_blocks.{i}.res", self.encoder.conv_blocks[i].res, g, B, tape, inv, flags)
                g = self._conv_bwd(f"encoder.conv_blocks.{i}.down", g, B, tape, inv, flags)
            self._conv_bwd("encoder.conv_first", g, B, tape, inv, flags, need_dx=False)        # the video needs no gradient
            out["grad_scale"] = S
            out["finite"] = bool(torch.stack(flags).all().item())
        return out

    def train_step(self, x, optimizer, grad_scale=None, **draws):
        """one step of the reference's recipe before `discriminator_iter_start`: `optimizer.zero_grad()`,
        `recon_backward(x, update_codebook=True)`, `optimizer.step()` -> recon_backward's dict.  A non-finite gradient raises before the
        optimizer step (the codebook has been updated by then: it saw only the forward).  `draws`: recon_backward's restart_src /
        restart_noise / init_src / init_noise / generator / frame_idx."""
        optimizer.zero_grad()
        out = self.recon_backward(x, grad_scale=grad_scale, update_codebook=True, **draws)
        if not out["finite"]:
            raise FloatingPointError(f"train_step: a gradient is not finite at grad_scale {out['grad_scale']:g}; the optimizer step was not taken "
                                     "(pass a smaller power-of-two grad_scale)")
        optimizer.step()
        return out

    def configure_optimizers(self):
        """the reference's autoencoder optimizer (vqgan.py:198-206; the codebook has buffers, no parameters); the discriminators'
        optimizer belongs to the follow-up"""
        params = (list(self.encoder.parameters()) + list(self.decoder.parameters()) + list(self.pre_vq_conv.parameters())
                  + list(self.post_vq_conv.parameters()) + list(self.codebook.parameters()))
        return torch.optim.Adam(params, lr=self._hp("lr", 3e-4), betas=(0.5, 0.9))

    # ---- validation (vqgan.py:190-196) on the metric operators of csrc/recon/recon.hip ---------------------------------------------------
    def _hp(self, name, default):
        a = self.args
        return a.get(name, default) if isinstance(a, dict) else getattr(a, name, default)

    def log(self, name, value, **kwargs):
        """pl.LightningModule.log for a module that runs without a trainer: the last value of every name, in `self.logged`"""
        self.__dict__.setdefault("logged", {})[name] = value

    @torch.no_grad()
    def reconstruct_stats(self, x, clip_u8=None, lpips_every=0):
        """x float32 [B, 3, T, H, W] on the GPU -> the reconstruction and the sums its quality figures are made of, all on the device:
        `recon` (decode(encode(x))), `ids`, `abs_sum` [B] = sum |recon - x|, `hist` [n_codes] of this batch's ids, `commit_sq_sum` [1] =
        sum |z - e|^2, `sq_err` / `ssim` [B, T] per frame of the byte clips `real_u8` / `recon_u8` [B, T, H, W, 3].  The bytes of both sides
        are `frames.video_to_clip_u8`'s, what the sampling scripts save and FVD reads; `clip_u8` hands in the real side's when the
        caller has them already (a raw batch's `to_clip_u8()`: the same bytes).  `frame_bytes` and `z_values` are the element counts
        the means divide by.  `lpips_every` = k > 0 adds `lpips` float64 [B, ceil(T / k)]: LPIPS(x, recon) of frames 0, k, 2k, ... of every
        clip on the float tensors (it needs the checkpoint's perceptual weights: `self.lpips`)."""
        from . import recon
        from .frames import video_to_clip_u8
        x = x.to(torch.float32).contiguous()
        B = x.shape[0]
        ids = self.encode(x)
        z = self._last_z
        rec = self.decode(ids)
        hist, sq_sum = recon.code_stats(ids, z, self._prepared["emb"])
        real_u8 = video_to_clip_u8(x) if clip_u8 is None else clip_u8
        recon_u8 = video_to_clip_u8(rec)
        sq_err, ssim = recon.clip_quality_u8(real_u8, recon_u8)
        st = {"recon": rec, "ids": ids, "abs_sum": recon.abs_diff_sum(x.view(B, -1), rec.view(B, -1)), "hist": hist,
              "commit_sq_sum": sq_sum, "sq_err": sq_err, "ssim": ssim, "real_u8": real_u8, "recon_u8": recon_u8,
              "frame_bytes": int(np.prod(real_u8.shape[2:])), "z_values": z.numel()}
        if lpips_every:
            if lpips_every < 0:
                raise ValueError(f"reconstruct_stats: lpips_every must be >= 0, got {lpips_every}")
            net = self.lpips
            if net is None:
                raise RuntimeError("reconstruct_stats: lpips_every needs the perceptual weights (a checkpoint with perceptual_model.* tensors, "
                                   "or `lpips_weights` set from mebt_amd.lpips.read_file)")
            ts = list(range(0, x.shape[2], int(lpips_every)))
            st["lpips"] = net(x, rec, frames=[(b, t) for b in range(B) for t in ts]).view(B, len(ts))
        return st

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """VQGAN.validation_step (vqgan.py:190-196): logs and returns val/recon_loss = mean |x_recon - x| * l1_weight, val/commitment_loss
        = 0.25 * mean (z - e)^2 and val/perplexity of the batch (0-dim float64 tensors on the device).  val/perceptual_loss: with
        perceptual_weight 0 (the reference's default) it is 0 and nothing is drawn.  Otherwise, when the checkpoint carried the
        perceptual weights (`self.lpips`), one frame per clip is drawn after the reconstruction as the reference draws it
        (`torch.randint(0, T, [B])` on the default CPU generator, vqgan.py:104, its only random call on this path) and the value is
        mean_b LPIPS(x[b, :, idx_b], recon[b, :, idx_b]) * perceptual_weight.  The reference would hand Lightning the [B, 1, 1, 1] tensor,
        which it accepts at B = 1 only; the mean equals it there.  Without the weights the term is left out, with a notice."""
        from . import recon
        from .frames import to_device_video
        x = to_device_video(batch["video"], self.codebook.embeddings.device)
        st = self.reconstruct_stats(x)
        out = {"val/recon_loss": st["abs_sum"].sum() / st["recon"].numel() * float(self._hp("l1_weight", 4.0)),
               "val/commitment_loss": 0.25 * st["commit_sq_sum"][0] / st["z_values"],
               "val/perplexity": recon.perplexity_of(st["hist"])}
        pw = float(self._hp("perceptual_weight", 0.0))
        if pw == 0.0:
            out["val/perceptual_loss"] = torch.zeros((), device=x.device, dtype=torch.float64)
        elif self.lpips is not None:
            frame_idx = torch.randint(0, x.shape[2], [x.shape[0]])
            out["val/perceptual_loss"] = self.lpips(x, st["recon"], frames=frame_idx).mean() * pw
        else:
            print("validation_step: val/perceptual_loss is left out (LPIPS is not built)")
        for k, v in out.items():
            self.log(k, v, prog_bar=True)
        return out


def load_vqgan(vqgan_ckpt, device=torch.device('cpu')):
    """reference download.py:50-54"""
    vqgan = VQGAN.load_from_checkpoint(vqgan_ckpt).to(device)
    vqgan.eval()
    return vqgan
