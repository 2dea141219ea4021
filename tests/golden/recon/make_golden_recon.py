#!/usr/bin/env python3
"""Generate tests/golden/recon/recon_golden.npz by running the *real* reference first stage (build container only: needs the
reference checkout, see tests/golden/make_golden.py for the stand-ins of its third-party imports).

Per config of make_golden.VQGAN_CONFIGS (vq_micro, vq_c5), on the closed-form weights and video of the encode / decode fixtures: what
`VQGAN.validation_step` (mebt/vqgan.py:190-196) logs — recon_loss (l1_weight 4.0), commitment_loss, perplexity — and the token ids.
`VQGAN.forward` moves a tensor to CUDA (vqgan.py:104), so the figures are computed from its own submodules in the order of
vqgan.py:98-102: pre_vq_conv(encoder(x)), codebook(z), decoder(post_vq_conv(embeddings)), F.l1_loss.

Usage:  python tests/golden/recon/make_golden_recon.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as F

from tests.golden.make_golden import VQGAN_CONFIGS, build_reference_vqgan, install_stubs, vqgan_video


def main():
    install_stubs()
    torch.manual_seed(0)
    out = {}
    for name in VQGAN_CONFIGS:
        model, cfg, P = build_reference_vqgan(name)
        x = vqgan_video(name)
        with torch.no_grad():
            z = model.pre_vq_conv(model.encoder(x))
            vq_output = model.codebook(z)
            x_recon = model.decoder(model.post_vq_conv(vq_output['embeddings']))
            recon_loss = F.l1_loss(x_recon, x) * model.l1_weight
        out[f"{name}_recon_loss"] = np.float64(recon_loss)
        out[f"{name}_commitment_loss"] = np.float64(vq_output['commitment_loss'])
        out[f"{name}_perplexity"] = np.float64(vq_output['perplexity'])
        out[f"{name}_ids"] = vq_output['encodings'].numpy()
        out[f"{name}_l1_weight"] = np.float64(model.l1_weight)
        print(name, {k: (float(v) if np.ndim(v) == 0 else v.shape) for k, v in out.items() if k.startswith(name)})
    path = os.path.join(os.environ.get("MEBT_GOLDEN_OUT", HERE), "recon_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
