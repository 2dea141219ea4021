"""Which kernel `mebt_op_conv3d` runs, asked of `mebt_conv3d_route` (csrc/vqgan.hip conv3d_route) on descriptors with null data
pointers: no GPU.  The expected names were read off the launcher's if-chain as it stood before it became a function and a table:

  f16 + MFMA, channels-last in, not NCDHW out, Cin % 32 == 0 and Cout % 64 == 0: the LDS-DMA kernel when also Cin % 64 == 0 (tile
      128 x 128 x 2 where Cout % 128 == 0, else 256 x 64 x 2), otherwise the register-staged `mfma_f16`;
  else f16 + MFMA, 3 -> 32 channels from the NCDHW video with 27 taps: `first_mfma`; channels-last Cin in {32, 64, 128} to Cout <= 16:
      `last_mfma_<Cin / 32>`;
  else, with MFMA allowed (either dtype), Cout <= 4 (Cin % 4 == 0 or NCDHW in): `voxel_4`; NCDHW in and Cout <= 32: `voxel_32`;
  else `direct` (always when MFMA is not allowed).

The environment knobs are read once per process, so each is checked in a fresh child."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPERATOR_CASES = [("conv", 3, (1, 1, 1), 32, 64), ("conv", 4, (2, 2, 2), 32, 64), ("conv", 4, (1, 2, 2), 64, 128), ("conv", 1, (1, 1, 1), 64, 64),
                  ("conv", 3, (1, 1, 1), 16, 24), ("conv", 3, (1, 1, 1), 64, 64), ("conv", 3, (1, 1, 1), 128, 256),
                  ("convt", 4, (2, 2, 2), 64, 64), ("convt", 4, (1, 2, 2), 128, 64), ("convt", 4, (2, 2, 2), 16, 8)]        # test_conv3d_operator's

# ---- config 5 (presets.vqgan_args(): 32 hidden channels, downsample (4, 8, 8), one 16 x 128 x 128 clip), f16 with MFMA ------------------
FWD_F16 = {
    "encoder.conv_first": "first_mfma",                                  # 3 -> 32, 27 taps, NCDHW fp32 in
    "encoder.conv_blocks.0.down": "mfma_f16",                            # 32 -> 64, k = 4, stride 2: Cin % 64 != 0
    "encoder.conv_blocks.0.res.conv1": "dma_256x64x2", "encoder.conv_blocks.0.res.conv2": "dma_256x64x2",       # 64 -> 64
    "encoder.conv_blocks.1.down": "dma_128x128x2",                       # 64 -> 128
    "encoder.conv_blocks.1.res.conv1": "dma_128x128x2", "encoder.conv_blocks.1.res.conv2": "dma_128x128x2",
    "encoder.conv_blocks.2.down": "dma_128x128x2",                       # 128 -> 256
    "encoder.conv_blocks.2.res.conv1": "dma_128x128x2", "encoder.conv_blocks.2.res.conv2": "dma_128x128x2",
    "pre_vq_conv": "dma_128x128x2",                                      # 256 -> 256, k = 1, fp32 channels-last out
    "post_vq_conv": "dma_128x128x2",
    "decoder.conv_blocks.0.up": "dma_128x128x2",                         # 256 -> 256 transposed: 8 classes of 8 taps
    "decoder.conv_blocks.0.res1.conv1": "dma_128x128x2", "decoder.conv_blocks.0.res1.conv2": "dma_128x128x2",
    "decoder.conv_blocks.0.res2.conv1": "dma_128x128x2", "decoder.conv_blocks.0.res2.conv2": "dma_128x128x2",
    "decoder.conv_blocks.1.up": "dma_128x128x2",                         # 256 -> 128
    "decoder.conv_blocks.1.res1.conv1": "dma_128x128x2", "decoder.conv_blocks.1.res1.conv2": "dma_128x128x2",
    "decoder.conv_blocks.1.res2.conv1": "dma_128x128x2", "decoder.conv_blocks.1.res2.conv2": "dma_128x128x2",
    "decoder.conv_blocks.2.up": "dma_256x64x2",                          # 128 -> 64, stride (1, 2, 2): 4 classes of 16 taps
    "decoder.conv_blocks.2.res1.conv1": "dma_256x64x2", "decoder.conv_blocks.2.res1.conv2": "dma_256x64x2",
    "decoder.conv_blocks.2.res2.conv1": "dma_256x64x2", "decoder.conv_blocks.2.res2.conv2": "dma_256x64x2",
    "decoder.conv_last": "last_mfma_2",                                  # 64 -> 3, fp32 NCDHW out
}
# the data gradient of a layer is a convolution Cout -> Cin of dy (channels-last in, fp32 channels-last out)
DGRAD_F16 = dict(FWD_F16)
DGRAD_F16.update({
    "encoder.conv_first": "last_mfma_1",                                 # 32 -> 3 (recon_backward never asks for it: the video needs no gradient)
    "encoder.conv_blocks.0.down": "direct",                              # 64 -> 32: Cout % 64 != 0 and too wide for the thin kernels
    "encoder.conv_blocks.1.down": "dma_256x64x2",                        # 128 -> 64
    "decoder.conv_blocks.2.up": "dma_128x128x2",                         # 64 -> 128
    "decoder.conv_last": "direct",                                       # 3 -> 64
})
# f32 with MFMA allowed: only the thin vector-ALU kernels are not `direct`
THIN_F32 = {("encoder.conv_first", "fwd"): "voxel_32", ("decoder.conv_last", "fwd"): "voxel_4", ("encoder.conv_first", "dgrad"): "voxel_4"}
OPERATOR_F16 = {0: "mfma_f16", 1: "mfma_f16", 2: "dma_128x128x2", 3: "dma_256x64x2", 4: "direct", 5: "dma_256x64x2", 6: "dma_128x128x2",
                7: "dma_256x64x2", 8: "dma_256x64x2", 9: "direct"}         # by index into OPERATOR_CASES


def _one_name(lib, code, descs, allow):
    names = {lib.mebt_conv3d_route(code, C.byref(d), allow) for d in descs}
    assert len(names) == 1 and None not in names, names                  # every class of a layer runs the same kernel
    return names.pop().decode()


def _layer_descs(cv, B, dims, in_mode=0, out_mode=0, resid=False):
    from mebt_amd.vqgan import _Desc
    od = cv.out_dims(dims)
    out = []
    for pi, taps, _ in cv.classes:
        d = _Desc.of(None, None, None, B, dims, cv.cin, od, cv.cout, cv.class_counts(od, pi), cv.os, pi, cv.sm, taps, in_mode, out_mode)
        d.resid = 8 if resid else None                                   # only whether it is set is read
        out.append(d)
    return out


def _dgrad_descs(cv, B, dims):
    from mebt_amd.vqgan import _Desc
    plan = cv.dgrad_plan(dims)
    return [_Desc.of(None, None, None, B, plan["zd"], cv.cout, plan["pd"], cv.cin, c["cq"], c["os"], c["pi"], c["sm"], c["taps"], 0, 1)
            for c in plan["classes"] if c["w"] is not None and min(c["cq"]) > 0]


def all_routes():
    """{"<dtype>/<allow_mfma>": {label: name}} over config 5 (forward and data gradient) and the operator test's ten shapes"""
    import torch
    from mebt_amd import _lib, presets
    from mebt_amd.vqgan import VQGAN, SamePadConv3d, SamePadConvTranspose3d, _Conv
    lib = C.CDLL(_lib.LIB_PATH)
    lib.mebt_conv3d_route.restype, lib.mebt_conv3d_route.argtypes = _lib.PROTOTYPES["mebt_conv3d_route"]
    args = presets.vqgan_args()
    m = VQGAN(args)
    B, video = 1, (args.sequence_length, args.resolution, args.resolution)
    out = {}
    for dtype, code in (("f16", _lib.F16), ("f32", _lib.F32)):
        m.compute_dtype = dtype
        m._prepared = None
        convs = {n: _Conv(mod.convt.weight if isinstance(mod, SamePadConvTranspose3d) else mod.conv.weight, None, mod.kernel_size, mod.stride,
                          isinstance(mod, SamePadConvTranspose3d), dtype)
                 for n, mod in m.named_modules() if isinstance(mod, (SamePadConv3d, SamePadConvTranspose3d))}
        # the launch plan of VQGAN._encode_z / decode: (layer, in_mode, out_mode, residual), dims threaded through
        plan = [("encoder.conv_first", 1, 0, False)]
        for i in range(len(m.encoder.conv_blocks)):
            plan += [(f"encoder.conv_blocks.{i}.down", 0, 0, False), (f"encoder.conv_blocks.{i}.res.conv1", 0, 0, False),
                     (f"encoder.conv_blocks.{i}.res.conv2", 0, 0, True)]
        plan += [("pre_vq_conv", 0, 1, False), ("post_vq_conv", 0, 0, False)]
        for i in range(len(m.decoder.conv_blocks)):
            plan.append((f"decoder.conv_blocks.{i}.up", 0, 0, False))
            for r in ("res1", "res2"):
                plan += [(f"decoder.conv_blocks.{i}.{r}.conv1", 0, 0, False), (f"decoder.conv_blocks.{i}.{r}.conv2", 0, 0, True)]
        plan.append(("decoder.conv_last", 0, 2, False))
        assert sorted(n for n, *_ in plan) == sorted(convs)
        for allow in (1, 0):
            got, dims = {}, video
            for name, in_mode, out_mode, resid in plan:
                cv = convs[name]
                got[name + ":fwd"] = _one_name(lib, code, _layer_descs(cv, B, dims, in_mode, out_mode, resid), allow)
                got[name + ":dgrad"] = _one_name(lib, code, _dgrad_descs(cv, B, dims), allow)
                dims = cv.out_dims(dims)
            assert dims == video                                          # the decoder undid the encoder's strides
            for i, (kind, k, stride, cin, cout) in enumerate(OPERATOR_CASES):
                w = torch.zeros((cout, cin, k, k, k) if kind == "conv" else (cin, cout, k, k, k))
                cv = _Conv(w, None, (k, k, k), stride, kind == "convt", dtype)
                got[f"op{i}"] = _one_name(lib, code, _layer_descs(cv, 2, (4, 6, 10)), allow)
                got[f"op{i}:resid_fp32out"] = _one_name(lib, code, _layer_descs(cv, 2, (4, 6, 10), 0, 1, True), allow)
            out[f"{dtype}/{allow}"] = got
    return out


def expected(dma=True, thin_mfma=True, tile=None):
    """the pinned names, and what the three knobs moved in the if-chain: MEBT_CONV_DMA=0 sends every LDS-DMA route to `mfma_f16`,
    MEBT_CONV_THIN_MFMA=0 the thin MFMA routes to the voxel kernel of their width, MEBT_CONV_TILE a tile to every LDS-DMA route whose
    Cout it divides (64 divides all of them here)"""
    def knobs(name):
        if name.startswith("dma_"):
            return "mfma_f16" if not dma else (tile or name)
        if not thin_mfma and name == "first_mfma":
            return "voxel_32"
        if not thin_mfma and name.startswith("last_mfma"):
            return "voxel_4"
        return name
    f16 = {n + ":fwd": knobs(v) for n, v in FWD_F16.items()}
    f16.update({n + ":dgrad": knobs(v) for n, v in DGRAD_F16.items()})
    for i, v in OPERATOR_F16.items():
        f16[f"op{i}"] = f16[f"op{i}:resid_fp32out"] = knobs(v)
    direct = {k: "direct" for k in f16}
    f32 = dict(direct)
    f32.update({f"{n}:{side}": v for (n, side), v in THIN_F32.items()})
    return {"f16/1": f16, "f16/0": direct, "f32/1": f32, "f32/0": direct}


def _in_child(env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MEBT_CONV_")}
    env.update(env_extra)
    code = "import json; from tests import test_vqgan_route_host as t; print('ROUTES ' + json.dumps(t.all_routes()))"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("ROUTES ")][-1][7:])


def _same(got, want):
    for leg in want:
        diff = {k: (got[leg].get(k), v) for k, v in want[leg].items() if got[leg].get(k) != v}
        assert not diff and set(got[leg]) == set(want[leg]), (leg, diff)


def test_routes_of_config_5_and_of_the_operator_shapes():
    _same(_in_child({}), expected())


@pytest.mark.parametrize("env,kw", [({"MEBT_CONV_DMA": "0"}, dict(dma=False)), ({"MEBT_CONV_THIN_MFMA": "0"}, dict(thin_mfma=False)),
                                    ({"MEBT_CONV_TILE": "256,64,3"}, dict(tile="dma_256x64x3"))])
def test_each_knob_moves_exactly_the_routes_it_moved(env, kw):
    want = expected(**kw)
    assert want != expected()
    _same(_in_child(env), want)


def test_route_refuses_what_the_operator_refuses_and_reads_no_data():
    from mebt_amd import _lib
    from mebt_amd.vqgan import _Desc
    lib = C.CDLL(_lib.LIB_PATH)
    lib.mebt_conv3d_route.restype, lib.mebt_conv3d_route.argtypes = _lib.PROTOTYPES["mebt_conv3d_route"]
    d = _Desc.of(None, None, None, 1, (2, 2, 2), 8, (2, 2, 2), 8, (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), [(0, 0, 0)], 0, 0)
    assert lib.mebt_conv3d_route(_lib.F32, C.byref(d), 1) == b"direct"
    assert lib.mebt_conv3d_route(_lib.BF16, C.byref(d), 1) is None and lib.mebt_conv3d_route(_lib.F32, None, 1) is None
    d.ntaps = 65
    assert lib.mebt_conv3d_route(_lib.F32, C.byref(d), 1) is None
    d.ntaps, d.B = 1, 0
    assert lib.mebt_conv3d_route(_lib.F32, C.byref(d), 1) == b"none"     # an empty class launches nothing
