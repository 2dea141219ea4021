"""Driver of tests/test_host_engine_route.py::test_workspace_layout_is_the_recorded_one: runs in a fresh subprocess with
MEBT_HOST_ONLY=1 (no GPU is touched) and prints, as one JSON object, mebt_workspace_bytes over descriptors x B x (NC, NT) x
training and mebt_kvcache_bytes per descriptor.  The descriptors: the five of tests/asan_host_driver.py and the ten-block mixed
list of tests/test_gpu_model.py::test_maskgit_blocks_rewrite_both_streams in both dtypes, each with dropout 0 and 0.1.
`python tests/workspace_bytes_driver.py > tests/golden/workspace_bytes.json` records the fixture."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mebt_amd import _lib  # noqa: E402

lib = _lib.load()
sky = ["latent_enc", "latent_self"] * 6 + ["latent_enc"] + ["latent_dec", "lt2l"] * 5 + ["latent_dec"]
mixed = ["latent_enc", "maskgit", "latent_self", "latent_enc", "latent_dec", "lt2l", "maskgit", "latent_enc", "latent_dec", "maskgit"]
DESCS = {"sky_1024_bf16": (24, 16, 1024, 256, 1024, _lib.BF16, sky), "sky_8192_bf16": (24, 16, 1024, 256, 8192, _lib.BF16, sky),
         "four_modes_f32": (4, 4, 256, 64, 256, _lib.F32, ["latent_enc", "latent_self", "latent_dec", "lt2l"]),
         "enc_dec_maskgit_bf16": (3, 2, 64, 8, 32, _lib.BF16, ["latent_enc", "latent_dec", "maskgit"]),
         "maskgit_only_f32": (2, 2, 128, 0, 64, _lib.F32, ["maskgit", "maskgit"]),
         "mixed10_f32": (10, 2, 64, 8, 32, _lib.F32, mixed), "mixed10_bf16": (10, 2, 64, 8, 32, _lib.BF16, mixed)}
out = {"workspace": {}, "kvcache": {}}
for name, (n_layer, n_head, d, ns, block, dtype, modes) in DESCS.items():
    for drop in (0.0, 0.1):
        m = _lib.ModelDesc()
        m.n_layer, m.n_head, m.n_embd, m.vocab, m.n_latent, m.block_size, m.dtype = n_layer, n_head, d, 16384, ns, block, dtype
        for i, mode in enumerate(modes):
            m.modes[i] = _lib.MODE_IDS[mode]
        m.label_smoothing, m.embd_pdrop, m.resid_pdrop, m.attn_pdrop = 0.0, drop, drop, drop
        h = C.c_void_p()
        assert lib.mebt_model_create(C.byref(m), C.byref(h)) == 0, lib.mebt_last_error()
        N = block
        for B in (1, 3, 6):
            for NC, NT in ((0, N), (N - 1, 1), (N // 2, N // 2), (N // 3, N - N // 3), (min(N, 7936), min(N, 256))):
                for training in (0, 1):
                    out["workspace"][f"{name} drop={drop} B={B} NC={NC} NT={NT} training={training}"] = lib.mebt_workspace_bytes(h, B, NC, NT, training)
        out["kvcache"][f"{name} drop={drop} B=2 N={N}"] = lib.mebt_kvcache_bytes(h, 2, N)
        lib.mebt_model_destroy(h)
print(json.dumps(out, indent=0, sort_keys=True))
