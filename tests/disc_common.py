"""Shared by tests/test_disc_host.py and tests/test_gpu_disc*.py: the golden file, the closed-form weights and the gates.

Gates (tests/golden/disc/make_golden_disc.py records the figures): F32 mode against the golden: four times the recorded fp32-vs-float64
distance of that tensor, relative to its maximum (both results are roundings of the same float64 value in different summation orders),
and where the recorded distance is below one fp32 rounding, that rounding; F16 mode: four times the recorded distance of the
fp16-storage twin from float64.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "disc")
sys.path.insert(0, GOLD)

from make_golden_disc import (CASES, D_KEYS, EPS32, G_KEYS, GAN_CASES, GAN_CONFIGS, ITER_START, SD_CONFIGS,  # noqa: E402,F401
                              closed_form_state_dict, gan_args, scalar_tolerances, structured_clip)

_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(os.path.join(GOLD, "disc_golden.npz")))
    return _gold


def stage_gate(stats_row, dtype):
    """absolute bound on a stage output's elements; stats_row = (distance32, distance16, max)"""
    d = max(stats_row[0], EPS32) if dtype == "f32" else stats_row[1]
    return 4.0 * d * stats_row[2]


def case_input(c):
    return structured_clip(CASES[c]["shape"])


def case_sd(c):
    cfg = CASES[c]
    return closed_form_state_dict(cfg["ndf"], cfg["L"], cfg["three_d"])


def reduce_dims(three_d):
    return (0, 2, 3, 4) if three_d else (0, 2, 3)


def check_against_golden(c, mode, dtype, logits, feats, report=print):
    """logits / feats in the reference's logical shapes (any device): every stage against the golden within the gate"""
    g, cfg = gold(), CASES[c]
    stats = g[f"{c}_{mode}_stats"]
    worst = 0.0
    for n, f in enumerate(feats):
        f = f.detach().double().cpu()
        assert tuple(f.shape) == tuple(g[f"{c}_{mode}_shape{n}"]), (c, mode, n, tuple(f.shape))
        gate = stage_gate(stats[n], dtype)
        if f"{c}_{mode}_feat{n}" in g:
            err = float((f - torch.from_numpy(g[f"{c}_{mode}_feat{n}"]).double()).abs().max())
        else:
            err = float((f.mean(reduce_dims(cfg["three_d"])) - torch.from_numpy(g[f"{c}_{mode}_cmean{n}"]).double()).abs().max())
        report(f"disc {c} {mode} {dtype} stage {n}: distance {err / stats[n][2]:.3e} of the maximum, gate {gate / stats[n][2]:.3e}")
        assert err <= gate, (c, mode, dtype, n, err, gate)
        worst = max(worst, err / gate)
    err = float((logits.detach().double().cpu() - torch.from_numpy(g[f"{c}_{mode}_logits"]).double()).abs().max())
    assert err <= stage_gate(stats[-1], dtype), (c, mode, dtype, "logits", err)
    return worst
