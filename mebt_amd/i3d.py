"""InceptionI3d — host-side mirror of reference mebt/fvd/pytorch_i3d.py (the Kinetics-400 I3D that FVD / KVD embed clips with)
on the HIP operators of csrc/i3d/i3d.hip.

The nn.Modules below only HOLD parameters, under the reference's module tree and state-dict names (`Conv3d_1a_7x7.conv3d.weight`,
`Mixed_3b.b1a.bn.running_var`, `logits.conv3d.bias`, ... 344 entries with `num_batches_tracked`), so a reference checkpoint loads
with strict=True.  `forward` walks a launch plan: every Unit3D is one `mebt_op_i3d_conv` (eval-mode BatchNorm, eps 1e-5, folded
into the weights and a bias in fp32 on the host), the three 1x1 branches of an Inception module that read its input (b0, b1a,
b2a) are ONE convolution whose epilogue writes b0 into its slice of the module's output and b1a / b2a into scratch, every other
branch writes straight into its slice (no concatenation), every MaxPool3dSamePadding is one `mebt_op_i3d_maxpool`, and the
AvgPool + logits + time mean is `mebt_op_i3d_head` in fp32.  Activations stay channels-last on the GPU; `compute_dtype` = "f16"
(MFMA, the default) or "f32" (parity).  Folding and the [Npad][Kpad] weight layout happen once, at the first call after a
(re)load.  No CPU / eager-torch compute path exists.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, ptr, cur_stream

BN_EPS = 1e-5                 # pytorch_i3d.py Unit3D: nn.BatchNorm3d(..., eps=1e-5)
TARGET_RESOLUTION = (224, 224)


class _Seg(C.Structure):
    _fields_ = [("out", C.c_void_p), ("n0", C.c_int32), ("n1", C.c_int32), ("cstride", C.c_int32), ("coff", C.c_int32)]


class _ConvDesc(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p),
                ("B", C.c_int32), ("Ti", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32), ("Cin", C.c_int32),
                ("To", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("Cout", C.c_int32),
                ("k", C.c_int32 * 3), ("s", C.c_int32 * 3), ("pad_front", C.c_int32 * 3), ("pad_back", C.c_int32 * 3),
                ("relu", C.c_int32), ("nseg", C.c_int32), ("seg", _Seg * 3)]


def same_pad(size, k, s):
    """TF "same" padding of pytorch_i3d.py compute_pad: (front, back, output size)"""
    pad = max(k - s, 0) if size % s == 0 else max(k - size % s, 0)
    return pad // 2, pad - pad // 2, -(-size // s)


def conv_geometry(dims, k, s):
    """per-axis (front, back, out) for a convolution / pool over dims (T, H, W)"""
    return [same_pad(d, kk, ss) for d, kk, ss in zip(dims, k, s)]


# ---- parameter holders ------------------------------------------------------------------------------------------------------
class Unit3D(nn.Module):
    """parameters of reference pytorch_i3d.py:50-136 (conv3d without bias, eval-mode BatchNorm; the logits unit: bias, no BN)"""

    def __init__(self, in_channels, output_channels, kernel_shape=(1, 1, 1), stride=(1, 1, 1), padding=0, activation_fn="relu",
                 use_batch_norm=True, use_bias=False, name='unit_3d'):
        super().__init__()
        self._kernel_shape, self._stride = tuple(kernel_shape), tuple(stride)
        self._use_batch_norm, self._relu = use_batch_norm, activation_fn is not None
        self.name = name
        self.conv3d = nn.Conv3d(in_channels, output_channels, self._kernel_shape, stride=self._stride, padding=0, bias=use_bias)
        if use_batch_norm:
            self.bn = nn.BatchNorm3d(output_channels, eps=BN_EPS, momentum=0.001)


class MaxPool3dSamePadding(nn.Module):
    """pytorch_i3d.py:13-46 (no parameters)"""

    def __init__(self, kernel_size, stride, padding=0):
        super().__init__()
        self.kernel_size, self.stride = tuple(kernel_size), tuple(stride)


class InceptionModule(nn.Module):
    """pytorch_i3d.py:140-170: out_channels = [c0, c1, c2, c3, c4, c5] -> concat(b0 c0, b1b c2, b2b c4, b3b c5)"""

    def __init__(self, in_channels, out_channels, name):
        super().__init__()
        c = out_channels
        self.out_channels = list(c)
        self.b0 = Unit3D(in_channels, c[0], [1, 1, 1], name=name + '/Branch_0/Conv3d_0a_1x1')
        self.b1a = Unit3D(in_channels, c[1], [1, 1, 1], name=name + '/Branch_1/Conv3d_0a_1x1')
        self.b1b = Unit3D(c[1], c[2], [3, 3, 3], name=name + '/Branch_1/Conv3d_0b_3x3')
        self.b2a = Unit3D(in_channels, c[3], [1, 1, 1], name=name + '/Branch_2/Conv3d_0a_1x1')
        self.b2b = Unit3D(c[3], c[4], [3, 3, 3], name=name + '/Branch_2/Conv3d_0b_3x3')
        self.b3a = MaxPool3dSamePadding([3, 3, 3], (1, 1, 1))
        self.b3b = Unit3D(in_channels, c[5], [1, 1, 1], name=name + '/Branch_3/Conv3d_0b_1x1')
        self.name = name


# (endpoint, kind, args) in the reference's order (pytorch_i3d.py:236-311)
_ENDPOINTS = [
    ('Conv3d_1a_7x7', 'unit', dict(cin=None, cout=64, k=(7, 7, 7), s=(2, 2, 2))),
    ('MaxPool3d_2a_3x3', 'pool', dict(k=(1, 3, 3), s=(1, 2, 2))),
    ('Conv3d_2b_1x1', 'unit', dict(cin=64, cout=64, k=(1, 1, 1), s=(1, 1, 1))),
    ('Conv3d_2c_3x3', 'unit', dict(cin=64, cout=192, k=(3, 3, 3), s=(1, 1, 1))),
    ('MaxPool3d_3a_3x3', 'pool', dict(k=(1, 3, 3), s=(1, 2, 2))),
    ('Mixed_3b', 'mixed', dict(cin=192, c=[64, 96, 128, 16, 32, 32])),
    ('Mixed_3c', 'mixed', dict(cin=256, c=[128, 128, 192, 32, 96, 64])),
    ('MaxPool3d_4a_3x3', 'pool', dict(k=(3, 3, 3), s=(2, 2, 2))),
    ('Mixed_4b', 'mixed', dict(cin=128 + 192 + 96 + 64, c=[192, 96, 208, 16, 48, 64])),
    ('Mixed_4c', 'mixed', dict(cin=192 + 208 + 48 + 64, c=[160, 112, 224, 24, 64, 64])),
    ('Mixed_4d', 'mixed', dict(cin=160 + 224 + 64 + 64, c=[128, 128, 256, 24, 64, 64])),
    ('Mixed_4e', 'mixed', dict(cin=128 + 256 + 64 + 64, c=[112, 144, 288, 32, 64, 64])),
    ('Mixed_4f', 'mixed', dict(cin=112 + 288 + 64 + 64, c=[256, 160, 320, 32, 128, 128])),
    ('MaxPool3d_5a_2x2', 'pool', dict(k=(2, 2, 2), s=(2, 2, 2))),
    ('Mixed_5b', 'mixed', dict(cin=256 + 320 + 128 + 128, c=[256, 160, 320, 32, 128, 128])),
    ('Mixed_5c', 'mixed', dict(cin=256 + 320 + 128 + 128, c=[384, 192, 384, 48, 128, 128])),
]


def launch_plan(T, H=224, W=224, in_channels=3, num_classes=400):
    """Host-only: the operator sequence of one forward for clips of T frames at H x W (after the resize), with every operator's
    input / output dims and TF-"same" pads.  Entries: dict(endpoint, op in {'conv', 'pool', 'mixed', 'head'}, ...).  The
    endpoint output dims (T, H, W, C) are what the reference's modules produce."""
    dims, ch = (T, H, W), in_channels
    plan = []
    for name, kind, a in _ENDPOINTS:
        if kind == 'unit':
            g = conv_geometry(dims, a['k'], a['s'])
            out = tuple(x[2] for x in g)
            plan.append(dict(endpoint=name, op='conv', in_dims=dims, out_dims=out, k=a['k'], s=a['s'], cin=ch, cout=a['cout'],
                             pad_front=tuple(x[0] for x in g), pad_back=tuple(x[1] for x in g)))
            ch = a['cout']
        elif kind == 'pool':
            g = conv_geometry(dims, a['k'], a['s'])
            out = tuple(x[2] for x in g)
            plan.append(dict(endpoint=name, op='pool', in_dims=dims, out_dims=out, k=a['k'], s=a['s'], cin=ch, cout=ch,
                             pad_front=tuple(x[0] for x in g), pad_back=tuple(x[1] for x in g)))
        else:
            c = a['c']
            g1 = conv_geometry(dims, (1, 1, 1), (1, 1, 1))
            g3 = conv_geometry(dims, (3, 3, 3), (1, 1, 1))
            out = dims
            plan.append(dict(endpoint=name, op='mixed', in_dims=dims, out_dims=out, cin=ch, cout=c[0] + c[2] + c[4] + c[5], c=list(c),
                             pad_front=tuple(x[0] for x in g3), pad_back=tuple(x[1] for x in g3),
                             pad1_front=tuple(x[0] for x in g1), pad1_back=tuple(x[1] for x in g1)))
            ch = c[0] + c[2] + c[4] + c[5]
        dims = out
    plan.append(dict(endpoint='Logits', op='head', in_dims=dims, out_dims=(dims[0] - 1, dims[1] - 6, dims[2] - 6), cin=ch,
                     cout=num_classes))
    return plan


def plan_flops(T, H=224, W=224, B=1):
    """algorithmic multiply-add FLOPs (2 per MAC) of the convolutions of one forward (the pools / head excluded: < 0.1 %)"""
    tot = 0
    for e in launch_plan(T, H, W):
        M = B * e['out_dims'][0] * e['out_dims'][1] * e['out_dims'][2]
        if e['op'] == 'conv':
            tot += 2 * M * e['cout'] * e['cin'] * e['k'][0] * e['k'][1] * e['k'][2]
        elif e['op'] == 'mixed':
            c, cin = e['c'], e['cin']
            tot += 2 * M * (cin * (c[0] + c[1] + c[3] + c[5]) + 27 * (c[1] * c[2] + c[3] * c[4]))
    return tot


class _Conv:
    """one prepared Unit3D (or the merged 1x1 of a module): folded weights [Npad][Kpad] of the compute dtype + fp32 bias"""

    def __init__(self, units, k, s, relu, dtype):
        ws, bs = [], []
        for u in units:
            w = u.conv3d.weight.detach().to(torch.float32)
            if u._use_batch_norm:
                bn = u.bn
                scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + BN_EPS)
                w = w * scale.view(-1, 1, 1, 1, 1)
                b = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
            else:
                b = u.conv3d.bias.detach().float() if u.conv3d.bias is not None else torch.zeros(w.shape[0], device=w.device)
            ws.append(w)
            bs.append(b)
        w = torch.cat(ws, 0)
        self.cout, self.cin = w.shape[0], w.shape[1]
        self.widths = [x.shape[0] for x in ws]
        K = self.cin * k[0] * k[1] * k[2]
        kpad, npad = -(-K // 32) * 32, -(-self.cout // 64) * 64
        wl = torch.zeros(npad, kpad, device=w.device, dtype=torch.float32)
        wl[:self.cout, :K] = w.permute(0, 2, 3, 4, 1).reshape(self.cout, K)            # [Cout][(dt, dh, dw, ci)]
        self.w = wl.to(torch.float16 if dtype == "f16" else torch.float32).contiguous()
        self.bias = torch.cat(bs).contiguous()
        self.k, self.s, self.relu = tuple(k), tuple(s), relu


def conv_launch(code, x, cv, B, in_dims, outs, relu=None):
    """x: channels-last [B, *in_dims, Cin]; outs: [(tensor, cstride, coff)] one per column segment of cv (widths cv.widths)"""
    g = conv_geometry(in_dims, cv.k, cv.s)
    d = _ConvDesc()
    d.in_, d.w, d.bias = ptr(x), ptr(cv.w), ptr(cv.bias)
    d.B, (d.Ti, d.Hi, d.Wi), d.Cin = B, in_dims, cv.cin
    d.To, d.Ho, d.Wo = (x_[2] for x_ in g)
    d.Cout = cv.cout
    for a in range(3):
        d.k[a], d.s[a], d.pad_front[a], d.pad_back[a] = cv.k[a], cv.s[a], g[a][0], g[a][1]
    d.relu = int(cv.relu if relu is None else relu)
    d.nseg = len(outs)
    n0 = 0
    for i, ((t, cstride, coff), wdt) in enumerate(zip(outs, cv.widths)):
        d.seg[i].out, d.seg[i].n0, d.seg[i].n1, d.seg[i].cstride, d.seg[i].coff = ptr(t), n0, n0 + wdt, cstride, coff
        n0 += wdt
    check(_lib.load().mebt_op_i3d_conv(_lib.F16 if code == "f16" else _lib.F32, C.byref(d), cur_stream()))
    return tuple(x_[2] for x_ in g)


def preprocess_uint8(videos, compute_dtype="f16"):
    """uint8 [B, T, H, W, 3] (a GPU tensor) -> channels-last [B, T, 224, 224, 3] of the compute dtype (fvd.py:preprocess)"""
    B, T, H, W, Cc = videos.shape
    if Cc != 3 or videos.dtype != torch.uint8:
        raise ValueError(f"expected uint8 videos [B, T, H, W, 3], got {videos.dtype} {tuple(videos.shape)}")
    videos = videos.contiguous()
    out = torch.empty(B, T, *TARGET_RESOLUTION, 3, device=videos.device, dtype=torch.float16 if compute_dtype == "f16" else torch.float32)
    check(_lib.load().mebt_op_i3d_preprocess(_lib.F16 if compute_dtype == "f16" else _lib.F32, ptr(videos), ptr(out), B * T, H, W,
                                             *TARGET_RESOLUTION, cur_stream()))
    return out


class InceptionI3d(nn.Module):
    """pytorch_i3d.py:173-338 with final_endpoint='Logits' (the FVD configuration: InceptionI3d(400, in_channels=3))"""

    VALID_ENDPOINTS = tuple(e[0] for e in _ENDPOINTS) + ('Logits', 'Predictions')

    def __init__(self, num_classes=400, spatial_squeeze=True, final_endpoint='Logits', name='inception_i3d', in_channels=3,
                 dropout_keep_prob=0.5):
        super().__init__()
        if final_endpoint != 'Logits':
            raise NotImplementedError("only final_endpoint='Logits' (what FVD uses) is built")
        self._num_classes, self.in_channels = num_classes, in_channels
        for ep, kind, a in _ENDPOINTS:
            if kind == 'unit':
                cin = in_channels if a['cin'] is None else a['cin']
                self.add_module(ep, Unit3D(cin, a['cout'], a['k'], a['s'], name=name + ep))
            elif kind == 'pool':
                self.add_module(ep, MaxPool3dSamePadding(a['k'], a['s']))
            else:
                self.add_module(ep, InceptionModule(a['cin'], a['c'], name + ep))
        self.logits = Unit3D(384 + 384 + 128 + 128, num_classes, [1, 1, 1], activation_fn=None, use_batch_norm=False, use_bias=True,
                             name='logits')
        self.compute_dtype = "f16"
        self._prepared = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_prepared", None))

    # ---- preparation ------------------------------------------------------------------------------------------------------
    def _prepare(self):
        dev = self.logits.conv3d.weight.device
        if dev.type != "cuda":
            raise RuntimeError("mebt_amd.i3d runs on MI355X only: move the model to the GPU (there is no CPU path in the product)")
        if self.compute_dtype not in ("f16", "f32"):
            raise ValueError(f"compute_dtype must be 'f16' or 'f32', not {self.compute_dtype!r}")
        key = (self.compute_dtype, dev)
        if self._prepared is not None and self._prepared["key"] == key:
            return self._prepared
        dt = self.compute_dtype
        prep = {"key": key}
        with torch.no_grad():
            for ep, kind, a in _ENDPOINTS:
                m = getattr(self, ep)
                if kind == 'unit':
                    prep[ep] = _Conv([m], m._kernel_shape, m._stride, True, dt)
                elif kind == 'mixed':
                    prep[ep] = dict(merged=_Conv([m.b0, m.b1a, m.b2a], (1, 1, 1), (1, 1, 1), True, dt),
                                    b1b=_Conv([m.b1b], (3, 3, 3), (1, 1, 1), True, dt),
                                    b2b=_Conv([m.b2b], (3, 3, 3), (1, 1, 1), True, dt),
                                    b3b=_Conv([m.b3b], (1, 1, 1), (1, 1, 1), True, dt))
            lw = self.logits.conv3d.weight.detach().float()
            prep["logits_w"] = lw.reshape(lw.shape[0], -1).contiguous()
            prep["logits_b"] = self.logits.conv3d.bias.detach().float().contiguous()
        self._prepared = prep
        return prep

    def _tdt(self):
        return _lib.torch_dtype(self.compute_dtype)

    # ---- operators --------------------------------------------------------------------------------------------------------
    def _pool(self, x, B, dims, k, s):
        od = tuple(-(-d // ss) for d, ss in zip(dims, s))
        out = torch.empty(B, *od, x.shape[-1], device=x.device, dtype=x.dtype)
        check(_lib.load().mebt_op_i3d_maxpool(self._code(), ptr(x), ptr(out), B, *dims, x.shape[-1], *k, *s, cur_stream()))
        return out, od

    def _code(self):
        return _lib.dtype_code(self.compute_dtype)

    def _unit(self, cv, x, B, dims):
        g = conv_geometry(dims, cv.k, cv.s)
        od = tuple(e[2] for e in g)
        out = torch.empty(B, *od, cv.cout, device=x.device, dtype=self._tdt())
        conv_launch(self.compute_dtype, x, cv, B, dims, [(out, cv.cout, 0)])
        return out, od

    def _mixed(self, p, c, x, B, dims):
        ctot = c[0] + c[2] + c[4] + c[5]
        dev, tdt = x.device, self._tdt()
        out = torch.empty(B, *dims, ctot, device=dev, dtype=tdt)
        s1 = torch.empty(B, *dims, c[1], device=dev, dtype=tdt)
        s2 = torch.empty(B, *dims, c[3], device=dev, dtype=tdt)
        conv_launch(self.compute_dtype, x, p["merged"], B, dims, [(out, ctot, 0), (s1, c[1], 0), (s2, c[3], 0)])
        conv_launch(self.compute_dtype, s1, p["b1b"], B, dims, [(out, ctot, c[0])])
        conv_launch(self.compute_dtype, s2, p["b2b"], B, dims, [(out, ctot, c[0] + c[2])])
        pooled, _ = self._pool(x, B, dims, (3, 3, 3), (1, 1, 1))
        conv_launch(self.compute_dtype, pooled, p["b3b"], B, dims, [(out, ctot, c[0] + c[2] + c[4])])
        return out

    def preprocess_uint8(self, videos):
        return preprocess_uint8(videos, self.compute_dtype)

    def forward_channels_last(self, x):
        """x: channels-last [B, T, H, W, 3] of the compute dtype on the GPU -> logits fp32 [B, num_classes]"""
        p = self._prepare()
        B, dims = x.shape[0], tuple(x.shape[1:4])
        for ep, kind, a in _ENDPOINTS:
            if kind == 'unit':
                x, dims = self._unit(p[ep], x, B, dims)
            elif kind == 'pool':
                x, dims = self._pool(x, B, dims, a['k'], a['s'])
            else:
                x = self._mixed(p[ep], a['c'], x, B, dims)
        Cc = x.shape[-1]
        if dims[0] < 2 or dims[1:] != (7, 7):
            raise ValueError(f"the logits head needs a [>= 2, 7, 7] feature map (clips of >= 9 frames at 224 x 224), got {dims}")
        pooled = torch.empty(B, dims[0] - 1, Cc, device=x.device, dtype=torch.float32)
        logits = torch.empty(B, self._num_classes, device=x.device, dtype=torch.float32)
        check(_lib.load().mebt_op_i3d_head(self._code(), ptr(x), ptr(p["logits_w"]), ptr(p["logits_b"]), ptr(pooled), ptr(logits), B,
                                           dims[0], dims[1], dims[2], Cc, self._num_classes, cur_stream()))
        return logits

    @torch.no_grad()
    def forward_uint8(self, videos):
        """uint8 videos [B, T, H, W, 3] (any H, W; a GPU tensor) -> logits [B, num_classes]: the resize runs on the GPU"""
        self._prepare()
        return self.forward_channels_last(self.preprocess_uint8(videos))

    @torch.no_grad()
    def forward(self, x):
        """reference forward: x float [B, 3, T, 224, 224] in [-1, 1] -> logits fp32 [B, num_classes]"""
        self._prepare()
        x = x.to(self.logits.conv3d.weight.device).permute(0, 2, 3, 4, 1).to(self._tdt()).contiguous()
        return self.forward_channels_last(x)
