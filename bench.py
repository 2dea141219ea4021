#!/usr/bin/env python3
"""Headline benchmark of the MeBT hot path on MI355X (contract: see the task's bench.py section).

metric  : masked video tokens/sec/GPU, train step (BASELINE.json `metric`)
workload: Sky-Timelapse 16f config (BASELINE.json configs[1]): 24L / d=1024 / 16 heads, 1024 VQ
          tokens + 256 latents, batch 6 per GPU, t = 0.5 -> NC = NT = 512 (SURVEY.md §8d headline
          point), synthetic token grids, random-init weights, dropout 0.1 as the config trains.
step    : embed -> 24 blocks -> head -> masked-token CE (+top-1/5) -> full backward ->
          (reduce-scatter / sharded AdamW / all-gather when N>1) -> AdamW.  Inputs are resident in HBM
          before timing starts.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]
  python bench.py --full [--windows 3] [--secondary none|light|full|c4|c5] [--no-cpu-baseline] ...
  (--secondary c4 / c5: ONLY that configuration's legs, no headline step — the process a rocprofv3 profile of config 4 / 5 wraps)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Rank 0 prints ONE JSON line.  A plain run sets up, runs one untimed step (GEMM tuner), the warm-up, ONE window of
exactly --steps timed steps, and prints the headline (`value`, `ms_per_step`); --dump-outputs DIR writes what the
last timed step computed (dump_outputs).  Everything else is measured only with --full, outside the timed window:
more windows (spread, GPU clocks), `host_enqueue_ms_per_step`, `roofline` = the GEMM kernel family (93 % of the
step's FLOPs), achieved = algorithmic FLOPs / HIP-event time on the launch stream; the data-parallel
self-description; `cpu_baseline` = the CPU oracle (kind "port") timed on this box's host cores on a bounded
sample of the same workload; `secondary` (N = 1 only) = the other metrics of SURVEY.md §8(d): the step with the
separate optimizer (what every data-parallel rank runs), the eval forward, the t sweep, a variable-t run, the
samplers at C2, the C4 revise schedule and the HBM rate of the embedding gather / scatter kernels.
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0     # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0         # HBM3E spec (6.29 TB/s measured with a float4 copy, same guide)
TRAFFIC_FILES = ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json")     # committed rocprofv3 --pmc summaries, newest first


def synthetic_batch(B, shape, rank, device):
    g = torch.Generator().manual_seed(1234 + rank)
    N = shape[0] * shape[1] * shape[2]
    x = torch.randint(0, 16384, (B, *shape), generator=g)
    idx = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
    return x.to(device), idx.to(device)


DUMP_SAMPLES = {"W": 4 << 20, "P": 1 << 20}      # fp32 elements of the updated weights written by --dump-outputs (20 MB)


def dump_outputs(out_dir, stats, native):
    """What the timed step hands its caller, after the last timed step: the statistics row TrainLoop.step returns
    ([CE sum, #top-1, #top-5, #rows, loss], float64) and the fp32 master weights it updated in place — the Linear
    weights W and the other parameters P, each whole if small, else a fixed sample (seeded positions, the same in every
    run with the same arguments)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "step_stats.npy"), stats.detach().double().cpu().numpy())
    g = torch.Generator().manual_seed(20240601)
    for name, flat in (("W", native.W), ("P", native.P)):
        n, k = flat.numel(), DUMP_SAMPLES[name]
        pos = torch.arange(n) if n <= k else torch.randint(0, n, (k,), generator=g).sort().values
        np.save(os.path.join(out_dir, f"master_{name}_sample.npy"), flat[pos.to(flat.device)].float().cpu().numpy())


def cpu_model_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return ""


def cpu_baseline(model_sd, cfg, t, sample_B=6):
    """The CPU oracle (a port of the reference algorithm, pinned to it by tests/golden) timed on this box's host cores: full
    train steps (fwd + CE + bwd + AdamW) of the same network at batch `sample_B` and the same t.  Thread counts 16 and 64 are
    timed (`value` = the faster); a count whose first step is already > 3x slower than the best so far is recorded from that
    one step and not repeated.  Counts above 64 are not run: on the 2 x 64-core / 256-thread EPYC 9575F hosts of this pool
    torch's CPU kernels at 256 threads measured 6.9 masked tokens/s against 700 at 16 (445 s per step, round-2 run
    gpurun_out/r2e) — it only burns the bounded budget of this leg."""
    from oracle import mebt_oracle as orc
    p = cfg.model.params
    ocfg = orc.OracleConfig(p.n_layer, p.n_head, p.n_embd, p.block_size, p.sos_emb, p.mode, shape=cfg.model.mask.params.shape,
                            schedule=cfg.model.mask.params.schedule, budget=cfg.model.mask.params.budget, avg_loss=1.0)
    ncpu = os.cpu_count() or 1
    st = orc.TrainState({k: v.float().cpu() for k, v in model_sd.items()}, lr=cfg.exp.exact_lr)
    x, idx = synthetic_batch(sample_B, cfg.model.mask.params.shape, 0, "cpu")
    runs = {}
    for threads in sorted({min(16, ncpu), min(64, ncpu)}):
        torch.set_num_threads(threads)
        t0 = time.perf_counter()
        r = orc.train_step(st, ocfg, x, idx, t)                  # warm-up step (allocator, thread pool); timed only as a guard
        warm = time.perf_counter() - t0
        if runs and warm > 3.0 * min(v[0] for v in runs.values()):
            runs[threads] = (warm, r["n_targets"])              # oversubscribed: one step is enough to show it
            continue
        dts = []
        for _ in range(2):
            t0 = time.perf_counter()
            r = orc.train_step(st, ocfg, x, idx, t)
            dts.append(time.perf_counter() - t0)
        runs[threads] = (min(dts), r["n_targets"])
    best = min(runs, key=lambda k: runs[k][0])
    dt, ntg = runs[best]
    return {"value": ntg / dt, "unit": "masked tokens/s", "cores": best, "kind": "port", "os_cpu_count": ncpu,
            "by_threads": {str(k): round(v[1] / v[0], 1) for k, v in runs.items()},
            "cores_note": f"{best} of {ncpu} hardware threads on purpose: `value` is the FASTEST thread count tried (by_threads); torch's CPU kernels "
                          "get slower beyond it on these hosts (256 threads: 6.9 masked tokens/s, round 2)",
            "sample": f"best of 2 timed train steps (fwd+CE+bwd+AdamW, after 1 warm-up) per thread count at batch {sample_B}, "
                      f"NC=NT={ntg // sample_B}, fp32, torch {torch.__version__} CPU, {cpu_model_name()} (os.cpu_count() = {ncpu}); "
                      f"{dt:.1f} s per step at {best} threads"}


def gpu_state(index=0):
    """Clocks / power / temperature of the GPU as the driver reports them (sysfs of the amdgpu device, `rocm-smi` as a fallback) -
    read OUTSIDE the timed region, before and after it, so that a swing of the headline between boxes or runs shows its cause in the
    line itself.  Every field is best effort: None where this user may not read it."""
    import glob
    st = {}
    cards = sorted(glob.glob("/sys/class/drm/card[0-9]*/device"))
    cards = [c for c in cards if os.path.exists(os.path.join(c, "pp_dpm_sclk"))]
    dev = cards[index] if index < len(cards) else (cards[0] if cards else None)

    def active(path):
        try:
            with open(path) as f:
                lines = f.read().strip().splitlines()
            cur = [ln for ln in lines if ln.rstrip().endswith("*")]
            return (cur[0] if cur else lines[-1]).split(":", 1)[1].replace("*", "").strip()
        except (OSError, IndexError):
            return None

    def num(path, scale):
        try:
            with open(path) as f:
                return round(int(f.read().strip()) * scale, 1)
        except (OSError, ValueError):
            return None

    if dev:
        st["sclk"] = active(os.path.join(dev, "pp_dpm_sclk"))
        st["mclk"] = active(os.path.join(dev, "pp_dpm_mclk"))
        st["fclk"] = active(os.path.join(dev, "pp_dpm_fclk"))
        st["perf_level"] = (lambda p_: open(p_).read().strip() if os.path.exists(p_) else None)(os.path.join(dev, "power_dpm_force_performance_level"))
        for hw in glob.glob(os.path.join(dev, "hwmon", "hwmon*")):
            st["power_cap_w"] = num(os.path.join(hw, "power1_cap"), 1e-6)
            st["power_avg_w"] = num(os.path.join(hw, "power1_average"), 1e-6) or num(os.path.join(hw, "power1_input"), 1e-6)
            st["temp_c"] = num(os.path.join(hw, "temp1_input"), 1e-3)
            break
    if not st.get("sclk"):
        try:
            import subprocess
            r = subprocess.run(["rocm-smi", "-d", str(index), "--showclocks", "--showpower", "--showtemp", "--json"], capture_output=True, text=True, timeout=20)
            st["rocm_smi"] = json.loads(r.stdout) if r.stdout.strip().startswith("{") else r.stdout[-400:]
        except Exception as e:          # noqa: BLE001
            st["rocm_smi"] = f"{type(e).__name__}: {e}"
    return st


class ClockSampler:
    """sclk / average power sampled from sysfs every 25 ms on a host thread while the timed windows run (the values before / after
    the windows are idle readings: the GPU clocks down within milliseconds).  Reads files only - nothing touches the GPU queue."""

    def __init__(self, index=0, period=0.025):
        import glob
        import threading
        cards = sorted(c for c in glob.glob("/sys/class/drm/card[0-9]*/device") if os.path.exists(os.path.join(c, "pp_dpm_sclk")))
        self.dev = cards[index] if index < len(cards) else (cards[0] if cards else None)
        hw = glob.glob(os.path.join(self.dev, "hwmon", "hwmon*")) if self.dev else []
        self.power = next((os.path.join(h, f) for h in hw for f in ("power1_average", "power1_input") if os.path.exists(os.path.join(h, f))), None)
        self.period, self.sclk, self.watts = period, [], []
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self._stop.is_set():
            try:
                with open(os.path.join(self.dev, "pp_dpm_sclk")) as f:
                    cur = [ln for ln in f.read().splitlines() if ln.rstrip().endswith("*")]
                if cur:
                    self.sclk.append(int("".join(ch for ch in cur[0].split(":", 1)[1] if ch.isdigit())))
                if self.power:
                    with open(self.power) as f:
                        self.watts.append(int(f.read().strip()) * 1e-6)
            except (OSError, ValueError, IndexError):
                pass
            self._stop.wait(self.period)

    def __enter__(self):
        if self.dev:
            self._thread.start()
        return self

    def __exit__(self, *a):
        self._stop.set()
        if self.dev:
            self._thread.join(timeout=1.0)

    def summary(self):
        if not self.sclk:
            return None
        s_ = sorted(self.sclk)
        out = {"samples": len(s_), "sclk_mhz": {"min": s_[0], "median": s_[len(s_) // 2], "max": s_[-1]}}
        if self.watts:
            out["power_w"] = {"mean": round(sum(self.watts) / len(self.watts), 1), "max": round(max(self.watts), 1)}
        return out


def timed(fn, n, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    sync()
    return (time.perf_counter() - t0) / n


def secondary_metrics(args, cfg, model, loop, x, idx, device, lib, level):
    """SURVEY.md §8(d) secondary metrics, one GPU, outside the headline's timed region."""
    from mebt_amd import presets, _lib
    from mebt_amd.trainer import TrainLoop
    sync = torch.cuda.synchronize
    B = args.batch
    out = {}
    if level in ("c4", "c5"):                  # one configuration only (no model of the headline config exists in this process)
        return secondary_c4(args, device, lib) if level == "c4" else secondary_c5(args, device, lib)
    ocfg = cfg.model.params
    forward_flops_per_sample = presets.forward_flops_per_sample

    # (1) the step as a data-parallel rank runs it (gradients stored, separate AdamW): the honest weak-scaling denominator
    sep = TrainLoop(model, fused_optimizer=False)
    sep.step_count = loop.step_count
    for _ in range(3):
        sep.step(x, idx, t=args.t)
    dt = timed(lambda: sep.step(x, idx, t=args.t), 10, sync)
    out["separate_optimizer"] = {"ms_per_step": round(dt * 1e3, 3), "masked_tokens_per_s": round(B * 512 / dt, 1),
                                 "note": "fwd + CE + bwd (fp32 gradients stored) + streaming AdamW: the N = 1 equivalent of the per-rank work under data parallelism"}

    # (2) embedding gather forward / scatter-add backward: HBM rate from HIP events and algorithmic bytes; the GEMM family of the
    # same steps WITHOUT the optimizer inside the weight-gradient launches (the headline's `roofline` charges the fused AdamW
    # epilogue's HBM streaming to the GEMM family; this is the family's own MFMA rate)
    lib.mebt_profile_enable(1)
    for _ in range(6):
        sep.step(x, idx, t=args.t)
    sync()
    n, tms, fl = C.c_double(), C.c_double(), C.c_double()
    _lib.check(lib.mebt_profile_read(0, C.byref(n), C.byref(tms), C.byref(fl)))
    if n.value and tms.value:
        tf = fl.value / (tms.value * 1e-3) / 1e12
        out["separate_optimizer"]["gemm_family"] = {"bound": "mfma", "achieved": round(tf, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                                                    "frac": round(tf / PEAK_BF16_TFLOPS, 4), "launches_per_step": n.value / 6,
                                                    "gemm_ms_per_step": round(tms.value / 6, 3),
                                                    "note": "by HIP events, weight gradients stored as fp32 (no AdamW epilogue)"}
    emb = {}
    for fam, name in ((2, "fwd"), (3, "bwd")):
        n, ms, by = C.c_double(), C.c_double(), C.c_double()
        _lib.check(lib.mebt_profile_read(fam, C.byref(n), C.byref(ms), C.byref(by)))
        if n.value and ms.value:
            gbs = by.value / (ms.value * 1e-3) / 1e9
            emb[name] = {"us_per_launch": round(ms.value / n.value * 1e3, 2), "algorithmic_MB": round(by.value / n.value / 1e6, 2),
                         "GB_per_s": round(gbs, 1), "frac_of_hbm_peak": round(gbs / PEAK_HBM_GBS, 4)}
    lib.mebt_profile_enable(0)
    out["embed_gather"] = emb

    # (3) eval forward (reconstruct_mask path) at the headline shape
    model.eval()
    ci, ti = idx[:, :512].contiguous(), idx[:, 512:].contiguous()
    with torch.no_grad():
        for _ in range(3):
            model.reconstruct_mask(x, ci, ti)
        dt = timed(lambda: model.reconstruct_mask(x, ci, ti), 20, sync)
    fl = forward_flops_per_sample(ocfg, 512, 512) * B
    out["eval_forward"] = {"ms": round(dt * 1e3, 3), "masked_tokens_per_s": round(B * 512 / dt, 1), "tflops": round(fl / dt / 1e12, 1)}
    model.train()
    if level == "light":
        return out

    # (4) t sweep of the train step (fused optimizer, as the headline)
    sweep = {}
    for t in (0.1, 0.25, 0.5, 0.75, 0.9):
        for _ in range(2):
            st = loop.step(x, idx, t=t)
        dt = timed(lambda: loop.step(x, idx, t=t), 8, sync)
        nt = int(st[3].cpu()) // B                   # targets per sample: ceil((1 - t) * N) under the linear schedule
        fl = 3 * forward_flops_per_sample(ocfg, 1024 - nt, nt) * B
        sweep[str(t)] = {"NT": nt, "ms_per_step": round(dt * 1e3, 3), "masked_tokens_per_s": round(B * nt / dt, 1), "tflops": round(fl / dt / 1e12, 1)}
    out["t_sweep"] = sweep

    # (5) t ~ U(0,1) as in real training (random.seed(42), E[NT] = 513): first pass pays the GEMM tuner
    # for the (bucketed) signatures it has not seen, the second pass is the steady state
    rng = random.Random(42)
    ts = [rng.random() for _ in range(100)]           # the 100-step run of SURVEY.md §8d
    passes = []
    for _ in range(2):
        sync()
        t0 = time.perf_counter()
        rows = torch.zeros((), device=device, dtype=torch.float64)
        for t in ts:
            rows += loop.step(x, idx, t=t)[3]
        sync()
        el = time.perf_counter() - t0
        tot = float(rows.cpu())
        passes.append({"s": round(el, 3), "ms_per_step": round(el / len(ts) * 1e3, 3), "masked_tokens_per_s": round(tot / el, 1)})
    out["variable_t"] = {"steps": len(ts), "first_pass_incl_tuning": passes[0], "steady_state": passes[1]}

    # (6) samplers at C2 (cosine schedule as the sampling script sets it), batch 4
    model.eval()
    model.mask_sampler.schedule = "cosine"            # sample_vqgan_transformer_videos.py:189,219
    Bs = 4
    x0 = torch.zeros(Bs, *cfg.model.mask.params.shape, dtype=torch.long, device=device)
    with torch.no_grad():
        f = lambda: model.sample(x0, None, 1.0, None, None, 32, None, None, context_temperature=4.5, skips=False)
        f()
        dt = timed(f, 2, sync)
        out["sample_32_steps_c2"] = {"batch": Bs, "s": round(dt, 4), "sampler_steps_per_s": round(32 / dt, 1), "tokens_per_s": round(Bs * 1024 / dt, 1)}
        xr = torch.randint(0, 16384, (Bs, *cfg.model.mask.params.shape), device=device)
        f = lambda: model.draft_and_revise(xr, None, 8, 1.0, None, None, 2, 1.0, None, None, 2, True)
        f()
        dt = timed(f, 3, sync)
        out["revise_2x2_c2"] = {"batch": Bs, "s": round(dt, 4), "forwards": 4, "forwards_per_s": round(4 / dt, 1)}
    model.mask_sampler.schedule = cfg.model.mask.params.schedule
    model.train()

    del sep
    # (6b) the reference's own arithmetic: the same step on the exact-fp32 engine (every GEMM on v_mfma_f32_32x32x2_f32, fp32
    # attention; train_transformer.py sets no precision, so the reference trains in fp32) — parity-tested, here timed
    torch.manual_seed(0)
    fm = presets.build_model(cfg, compute_dtype="f32").to(device).train()
    fl = TrainLoop(fm, fused_optimizer=False)
    for _ in range(2):
        fl.step(x, idx, t=args.t)
    dt = timed(lambda: fl.step(x, idx, t=args.t), 5, sync)
    flops = 3 * forward_flops_per_sample(ocfg, 512, 512) * B
    out["fp32_step"] = {"ms_per_step": round(dt * 1e3, 3), "masked_tokens_per_s": round(B * 512 / dt, 1), "tflops": round(flops / dt / 1e12, 1),
                        "frac_of_fp32_mfma_peak": round(flops / dt / 1e12 / PEAK_F32_TFLOPS, 4),
                        "note": "exact-fp32 engine (the 1e-3 parity gate), separate AdamW; peak = 157.3 TFLOP/s fp32 MFMA"}
    del fm, fl
    torch.cuda.empty_cache()
    out.update(secondary_c4(args, device, lib))
    out.update(secondary_c5(args, device, lib))
    return out


def executed_rates(reference_flops, wall_s, share):
    """Rates of an inference leg whose loop SKIPS work the reference does (key / value cache): `reference_equivalent_tflops` divides the
    reference's algorithmic FLOPs by the time - how fast the leg is in the reference's currency, not a utilisation; the `executed_*`
    figures count only FLOPs of GEMM launches that ran (mebt_profile_read): by the launches' own HIP-event time (the family's MFMA
    roofline fraction) and by the leg's wall time (end to end: attention, LayerNorm, the draw and host gaps charged to them)."""
    ex, ms = share["gemm_tflop"] * 1e12, share["gemm_ms_by_events"]
    return {"reference_equivalent_tflops": round(reference_flops / wall_s / 1e12, 1),
            "executed_gemm_tflop": share["gemm_tflop"], "gemm_launches": share["gemm_launches"], "gemm_ms_by_events": ms,
            "executed_tflops": round(ex / max(ms, 1e-9) / 1e9, 1), "executed_frac": round(ex / max(ms, 1e-9) / 1e9 / PEAK_BF16_TFLOPS, 4),
            "executed_tflops_end_to_end": round(ex / wall_s / 1e12, 1), "executed_frac_end_to_end": round(ex / wall_s / 1e12 / PEAK_BF16_TFLOPS, 4),
            "executed_share_of_reference_flops": round(ex / reference_flops, 4)}


def secondary_c4(args, device, lib):
    """BASELINE.json configs[3]: UCF-101 128f geometry (block 8192), batch 4 as the shipped script runs it
    (scripts/valid_dnr_config_ckpt_exp_ucf_128f.sh:12,34) — the inference schedules and one train step.  `--c4-legs` selects."""
    from mebt_amd import presets, _lib
    from mebt_amd.trainer import TrainLoop
    from mebt_amd.sampling import bidirect_sample
    sync = torch.cuda.synchronize
    forward_flops_per_sample = presets.forward_flops_per_sample
    legs = set(args.c4_legs.split(","))
    out = {}
    ucfg = presets.ucf_128f()
    uo = ucfg.model.params
    torch.manual_seed(1)
    um = presets.build_model(ucfg, compute_dtype=args.dtype).to(device).eval()

    def gemm_share(fn):
        """GEMM-family launches of one more call bracketed by HIP events: their FLOPs and summed duration"""
        lib.mebt_profile_enable(1)
        fn()
        sync()
        n, tms, fl = C.c_double(), C.c_double(), C.c_double()
        _lib.check(lib.mebt_profile_read(0, C.byref(n), C.byref(tms), C.byref(fl)))
        lib.mebt_profile_enable(0)
        return {"gemm_launches": n.value, "gemm_tflop": round(fl.value / 1e12, 2), "gemm_ms_by_events": round(tms.value, 2),
                "gemm_family_tflops": round(fl.value / max(tms.value, 1e-9) / 1e9, 1)}

    if "revise" in legs:
        # the revise schedule of the shipped script: M = 2 x 32 revise forwards at (NC, NT) = (7936, 256)
        xu = torch.randint(0, 16384, (4, 32, 16, 16), device=device)
        with torch.no_grad():
            f = lambda: um.draft_and_revise(xu, None, 8, 1.0, None, None, 32, 1.0, None, None, 2, True)
            f()
            dt = timed(f, 1, sync)
            fl = 64 * 4 * forward_flops_per_sample(uo, 7936, 256)
            out["c4_revise_64_forwards"] = {"batch": 4, "s": round(dt, 3), "forwards_per_s": round(64 / dt, 1),
                                            **executed_rates(fl, dt, gemm_share(f)),
                                            "note": "64 forwards at (NC, NT) = (7936, 256) + sampling + scatter, block 8192.  reference_equivalent_tflops = the "
                                                    "reference's algorithmic FLOPs (every forward re-projects every context position) / time: a speed "
                                                    "figure, NOT a roofline fraction (the cached loop skips most of that work); executed_* count only the "
                                                    "FLOPs of GEMM launches that ran",
                                            "kv_cache": None if getattr(um, "_kv_last", None) is None else
                                            {"context_rows_projected": um._kv_last[0], "context_rows_uncached": um._kv_last[1],
                                             "note": "latent_enc keys / values of all positions cached per loop (mebt_forward_kvcache): only positions whose token changed are re-projected; MEBT_KV_CACHE=0 disables"}}
    if "sample" in legs:
        # the 30-step MaskGIT-style sample at the same geometry (the other C4 inference schedule), cosine mask
        # schedule as the sampling script sets it: NT shrinks from 8192 to 0 over the steps
        um.mask_sampler.schedule = "cosine"
        x0u = torch.zeros(4, 32, 16, 16, dtype=torch.long, device=device)
        with torch.no_grad():
            f = lambda: um.sample(x0u, None, 1.0, None, None, 30, None, None, context_temperature=4.5, skips=False)
            f()
            dt = timed(f, 1, sync)
        fl = 4 * 36.5e12
        out["c4_sample_30_steps"] = {"batch": 4, "s": round(dt, 3), "sampler_steps_per_s": round(30 / dt, 1), "tokens_per_s": round(4 * 8192 / dt, 1),
                                     **executed_rates(fl, dt, gemm_share(f)),
                                     "note": "reference-equivalent FLOPs = SURVEY.md §8d's 36.5 TFLOP per sample (uncached)"}
    if "bootstrap" in legs:
        # the shipped UCF-128f draft producer (scripts/valid_dnr_config_ckpt_exp_ucf_128f.sh:10-15 -> sample_vqgan_transformer_videos.py:22-94):
        # bidirect_sample with --bootstrap 64 --top_k 32, then 32 MaskGIT steps; FLOP model of SURVEY.md §8d (107.8 + 36.5 TFLOP/sample)
        um.mask_sampler.schedule = "cosine"
        with torch.no_grad():
            f = lambda: bidirect_sample(um, 4, 128, 128, 128, temperature=1.0, top_k=32, top_p=None, vid_n_steps=32, vid_c_temp=2.0, bootstrap=64)
            f()
            dt = timed(f, 1, sync)
            fl = 4 * (107.8e12 + 36.5e12)
            out["c4_bootstrap64_topk32"] = {"batch": 4, "s": round(dt, 3), "forwards": 96, "videos_per_s": round(4 / dt, 3),
                                            **executed_rates(fl, dt, gemm_share(f)),
                                            "note": "bidirect_sample(bootstrap=64, top_k=32, vid_n_steps=32, vid_c_temp=2.0) at block 8192 incl. the [4, 8192, 16384] "
                                                    "probability maps of debug=True; reference-equivalent FLOPs = SURVEY.md §8d's 107.8 + 36.5 TFLOP per sample (uncached)"}
    um.mask_sampler.schedule = ucfg.model.mask.params.schedule
    del um
    torch.cuda.empty_cache()
    if "train" in legs:
        # TRAINING at block 8192 (configs/ucf/mebt_128f.yaml:4-57): B = 4, t = 0.5 on the full sequence -> NC = NT = 4096
        torch.manual_seed(1)
        tm = presets.build_model(ucfg, compute_dtype=args.dtype).to(device).train()
        tm.t_prior = lambda lengths, step: __import__("numpy").eye(len(lengths))[-1]      # always the full 32 latent frames (the curriculum's end state)
        tl = TrainLoop(tm)
        xt, it = synthetic_batch(4, [32, 16, 16], 0, device)
        for _ in range(3):
            tl.step(xt, it, t=0.5)
        dt = timed(lambda: tl.step(xt, it, t=0.5), 5, sync)
        fl = 3 * 4 * forward_flops_per_sample(uo, 4096, 4096)
        share = gemm_share(lambda: tl.step(xt, it, t=0.5))          # the GEMM family of one more step by HIP events (incl. the fused AdamW epilogues)
        out["c4_train_step"] = {"batch": 4, "NC": 4096, "NT": 4096, "ms_per_step": round(dt * 1e3, 3), "masked_tokens_per_s": round(4 * 4096 / dt, 1),
                                "tflops": round(fl / dt / 1e12, 1), "frac_of_bf16_mfma_peak": round(fl / dt / 1e12 / PEAK_BF16_TFLOPS, 4),
                                "gemm_family": {"bound": "mfma", "achieved": share["gemm_family_tflops"], "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                                                "frac": round(share["gemm_family_tflops"] / PEAK_BF16_TFLOPS, 4), "gemm_ms_by_events": share["gemm_ms_by_events"],
                                                "gemm_tflop": share["gemm_tflop"], "launches": share["gemm_launches"],
                                                "note": "the same kernels as the headline at 16 384 rows per product: what the family reaches when the shapes "
                                                        "allow 256-wide tiles in whole rounds"},
                                "optimizer": "in-backward" if tl.fused_optimizer else "separate"}
        del tm, tl
        torch.cuda.empty_cache()
    return out


def secondary_c5(args, device, lib):
    """BASELINE.json configs[4]: Taichi 16f end to end, at the batch the shipped script runs (`--batch_size 16`,
    scripts/valid_dnr_config_ckpt_exp_taichi_16f.sh:12,34; rounds 1-3 timed batch 4: `--c5-batch 4` reproduces that figure)."""
    from mebt_amd import presets, _lib
    sync = torch.cuda.synchronize
    out = {}
    # (8) C5 (BASELINE.json configs[4]): Taichi 16f end to end — pixels -> 3D-VQGAN encode (fp16 MFMA, fp32 codebook search) ->
    # MeBT sampling as the shipped script runs it (64-step MaskGIT draft through bidirect_sample incl. its debug=True probability map,
    # then M = 8 x 2 revise forwards at T = 0.3) -> 3D-VQGAN decode, batch 16, random-init weights
    from mebt_amd.vqgan import VQGAN
    tcfg = presets.taichi_16f(vtokens=False)
    torch.manual_seed(2)
    tm = presets.build_model(tcfg, compute_dtype=args.dtype)
    tm.first_stage_model = VQGAN(presets.vqgan_args())
    tm.first_stage_model.compute_dtype = "f16"
    tm = tm.to(device).eval()
    tm.mask_sampler.schedule = "cosine"
    from mebt_amd.sampling import bidirect_sample
    Bv = args.c5_batch
    vid = torch.rand(Bv, 3, 16, 128, 128, device=device) - 0.5
    with torch.no_grad():
        stages = {}
        enc = lambda: tm.encode_to_z(vid)[1]
        toks = enc()
        stages["vqgan_encode_ms"] = round(timed(enc, 3, sync) * 1e3, 3)
        fs, tm.first_stage_model = tm.first_stage_model, None       # the draft's decode is timed as its own stage below
        draft = lambda: bidirect_sample(tm, Bv, 16, 16, 16, temperature=1.0, top_k=None, top_p=None, vid_n_steps=64, vid_c_temp=2.0,
                                        ctemp_schedule="linear", strategy="maskgit")["code_maps"]       # sample_vqgan_transformer_videos.py:22-94
        code = draft()
        stages["sample_64_steps_ms"] = round(timed(draft, 1, sync) * 1e3, 3)
        rev = lambda: tm.draft_and_revise(code.reshape(Bv, 4, 16, 16), None, 8, 0.0, None, None, 2, 0.3, None, None, 8, True)
        code2 = rev()
        stages["revise_8x2_ms"] = round(timed(rev, 1, sync) * 1e3, 3)
        tm.first_stage_model = fs
        dec = lambda: tm.first_stage_model.decode(code2.view(Bv, 4, 16, 16))
        rec = dec()
        stages["vqgan_decode_ms"] = round(timed(dec, 3, sync) * 1e3, 3)
        # per-stage roofline (MFMA-bound stages): the sampler stages once more with the GEMM family bracketed by HIP events —
        # exact algorithmic FLOPs of its launches and their summed duration; `achieved` = those FLOPs / the stage's wall time
        # (so it also charges attention, LayerNorm and the sampling kernels to the GEMMs: conservative)
        stage_roof = {}
        for name, fn in (("sample_64_steps", draft), ("revise_8x2", rev)):
            lib.mebt_profile_enable(1)
            fn()
            sync()
            n, tms, fl = C.c_double(), C.c_double(), C.c_double()
            _lib.check(lib.mebt_profile_read(0, C.byref(n), C.byref(tms), C.byref(fl)))
            lib.mebt_profile_enable(0)
            wall = stages[name + "_ms"] * 1e-3
            stage_roof[name] = {"bound": "mfma", "achieved": round(fl.value / wall / 1e12, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                                "frac": round(fl.value / wall / 1e12 / PEAK_BF16_TFLOPS, 4), "gemm_launches": n.value,
                                "gemm_gflop": round(fl.value / 1e9, 1), "gemm_ms_by_events": round(tms.value, 2)}
        for name, gflop in (("vqgan_encode", Bv * 2 * 23.83), ("vqgan_decode", Bv * 2 * 347.17)):
            tf = gflop / stages[name + "_ms"]                     # GFLOP / ms = TFLOP/s
            stage_roof[name] = {"bound": "mfma", "achieved": round(tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                                "frac": round(tf / PEAK_BF16_TFLOPS, 4), "conv_gflop": round(gflop, 1)}
    assert tuple(rec.shape) == (Bv, 3, 16, 128, 128) and tuple(toks.shape) == (Bv, 1024)
    total = sum(stages.values())
    stages.update({"batch": Bv, "total_ms": round(total, 2), "videos_per_s": round(Bv / (total * 1e-3), 2),
                   "vqgan_encode_tflops": round(Bv * 2 * 23.83e9 / (stages["vqgan_encode_ms"] * 1e-3) / 1e12, 1),
                   "vqgan_decode_tflops": round(Bv * 2 * 347.17e9 / (stages["vqgan_decode_ms"] * 1e-3) / 1e12, 1),
                   "roofline_by_stage": stage_roof,
                   "note": "16 frames x 128 x 128 per video; VQGAN fp16 (conv3d implicit GEMM on v_mfma_f32_16x16x32_f16), transformer " + args.dtype})
    out["c5_taichi_end_to_end"] = stages
    return out




def comm_env():
    """the communication-related environment actually in effect (so that a multi-GPU line is diagnosable on its own)"""
    env = {k: v for k, v in sorted(os.environ.items()) if k.startswith(("NCCL_", "RCCL_", "HSA_", "MEBT_DP_", "MEBT_OVERLAP", "TORCH_NCCL_"))}
    try:
        env["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception:          # noqa: BLE001
        env["rccl_version"] = None
    return env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--t", type=float, default=0.5)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs as DIR/<name>.npy (dump_outputs)")
    ap.add_argument("--full", action="store_true", help="also measure everything beyond the headline (module docstring)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU oracle baseline")
    ap.add_argument("--windows", type=int, default=None, help="--full: timed windows of --steps steps (default 3): the first is the judged one, the others report the spread")
    ap.add_argument("--secondary", default=None, choices=["none", "light", "full", "c4", "c5"], help="--full: which secondary legs run (default full)")
    ap.add_argument("--preset", default="sky_16f", choices=["sky_16f", "tiny"])
    ap.add_argument("--c5-batch", type=int, default=16, help="videos per batch of the config-5 leg (the shipped Taichi script: 16)")
    ap.add_argument("--c4-legs", default="revise,sample,bootstrap,train", help="which config-4 legs run (profiling one at a time)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full and (args.secondary not in (None, "none") or (args.windows or 1) > 1):
        ap.error("--secondary and more than one window measure beyond the headline: add --full")
    if args.dump_outputs and args.secondary in ("c4", "c5"):
        ap.error("--dump-outputs needs the headline step, which --secondary c4 / c5 does not run")
    if args.windows is None:
        args.windows = 3 if args.full else 1
    if args.secondary is None:
        args.secondary = "full" if args.full else "none"

    # `python bench.py --gpus N` without a torch.distributed environment: start the N ranks as a child process (before anything
    # here touches the GPU), relay rank 0's line, exit with the child's return code (mebt_amd/launch.py)
    from mebt_amd.launch import spawn_ranks_if_needed
    rc = spawn_ranks_if_needed(args.gpus, os.path.abspath(__file__), sys.argv[1:])
    if rc is not None:
        sys.exit(rc)

    # The contract is ONE JSON line on stdout.  RCCL prints a version banner through C stdio (block-buffered on a pipe, so
    # it would come out AFTER the result line at exit): keep the real stdout aside and point fd 1 at stderr for
    # everything else in this process, native libraries included.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    import torch.distributed as dist
    from mebt_amd import presets
    from mebt_amd.parallel import GradReducer
    from mebt_amd.trainer import TrainLoop
    from mebt_amd import _lib

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend = "nccl"                                      # RCCL
    if os.environ.get("MEBT_BENCH_SHARE_GPU") == "1":     # functional check of the N>1 path on a 1-GPU box: all ranks on GPU 0, gloo
        local_rank, backend = 0, "gloo"
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dp_force = world == 1 and os.environ.get("MEBT_DP_FORCE") == "1"    # one rank, but the whole N > 1 path: RCCL group of size 1, sharded reducer
    if world > 1 or dp_force:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        if backend == "nccl":
            from mebt_amd.parallel import init_rccl
            init_rccl(rank, world, device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"

    if args.secondary in ("c4", "c5"):        # profiling aid: only that configuration's legs run in this process, no headline step
        assert world == 1
        lib = _lib.load()
        sec = secondary_metrics(args, None, None, None, None, None, device, lib, args.secondary)
        os.write(real_stdout, (json.dumps({"metric": "secondary legs only (profiling run)", "value": None, "only": args.secondary, "dtype": args.dtype,
                                           "data": "synthetic", "secondary": sec}) + "\n").encode())
        return
    # the Sky config trains with embd/resid/attn dropout 0.1 (configs/stl/mebt_16f.yaml:12-14): the measured
    # step includes it (counter-based masks, recomputed in backward)
    cfg = presets.sky_16f(vtokens=True, dropout=args.dropout) if args.preset == "sky_16f" else presets.tiny()
    torch.manual_seed(0)                       # identical random-init weights on every rank
    model = presets.build_model(cfg, compute_dtype=args.dtype).to(device).train()
    reducer = GradReducer(world_size=world)
    loop = TrainLoop(model, reducer)
    shape = cfg.model.mask.params.shape
    x, idx = synthetic_batch(args.batch, shape, rank, device)
    dp_fallback = None
    if reducer.active and reducer.mode == "sharded":
        # The sharded path has only ever met RCCL with one rank on the build machines.  If its first step raises on a real
        # multi-GPU node (every rank runs the same calls, so every rank raises), fall back to the plain bucketed fp32
        # all-reduce with a replicated optimizer rather than produce no number; the JSON line carries `dp_fallback`.
        try:
            loop.step(x, idx, t=args.t)
            torch.cuda.synchronize()
            if os.environ.get("MEBT_BENCH_FAIL_SHARDED") == "1":      # tests: exercise the fallback below after a real (half-applied) sharded step
                raise RuntimeError("injected failure of the sharded data-parallel step (MEBT_BENCH_FAIL_SHARDED=1)")
        except Exception as e:          # noqa: BLE001
            dp_fallback = f"{type(e).__name__}: {e}"
            print(f"[bench] sharded data-parallel step failed ({dp_fallback}); falling back to MEBT_DP_MODE=allreduce", file=sys.stderr, flush=True)
            try:
                torch.cuda.synchronize()
            except Exception:           # noqa: BLE001
                pass
            reducer.abandon(loop.native)                     # drop half-issued work, forward waits, the bf16 wire-gradient binding
            torch.manual_seed(0)                             # the half-applied step touched some shards: start again from the
            model = presets.build_model(cfg, compute_dtype=args.dtype).to(device).train()   # same initial weights on every rank
            reducer = GradReducer(world_size=world, mode="allreduce")
            loop = TrainLoop(model, reducer)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    # initialisation, not warm-up: the first step of a process times the GEMM tuner's candidates in situ (seconds); it must never
    # land in the timed region, whatever --warmup says
    stats = loop.step(x, idx, t=args.t)
    sync()
    for _ in range(args.warmup):
        stats = loop.step(x, idx, t=args.t)
    if loop.sync_tune:                 # data parallel: the followers adopt rank 0's GEMM table now, and no table sync (a host read on
        reducer.sync_tune_table()      # every rank, i.e. a drained GPU queue) happens inside the timed region
        loop.hold_tune_sync = True
    sync()
    gpu_before = gpu_state(local_rank) if args.full and rank == 0 else None
    wire0 = reducer.bytes_on_wire

    def window():
        """EXACTLY --steps steps between barrier + synchronize on both sides, max over ranks"""
        sync()
        t0 = time.perf_counter()
        st_ = None
        for _ in range(args.steps):
            st_ = loop.step(x, idx, t=args.t)
        sync()
        el = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([el], device=device, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            el = float(tt.item())
        return el, st_

    sampler = ClockSampler(local_rank) if args.full and rank == 0 else None
    if sampler is not None:
        sampler.__enter__()
    elapsed, stats = window()            # THE timed region: `value` / `ms_per_step` come from this window alone
    wire1 = reducer.bytes_on_wire
    if args.dump_outputs:                # before any further step changes the weights
        loop.consolidate(optimizer_state=False)      # sharded data parallel: complete fp32 masters on every rank (a collective)
        if rank == 0:
            dump_outputs(args.dump_outputs, stats, loop.native)
        sync()
    stats = stats.cpu()
    n_targets = int(stats[3])                                  # masked tokens scored per rank per step
    ms = 1e3 * elapsed / args.steps
    value = world * n_targets * args.steps / elapsed
    wire_bytes_per_step = (wire1 - wire0) / max(1, args.steps)     # payload of the timed steps only
    out = {"metric": "masked video tokens/sec/GPU (train step, 24L d=1024, 1024+256 tok)",
           "value": round(value, 1), "unit": "masked tokens/s (whole job)", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
           "per_gpu": round(value / world, 1),
           "config": {"workload": "Sky-Timelapse 16f MeBT train step: 24L/1024d/16h, 1024 VQ tokens + 256 latents, "
                                  f"batch {args.batch}/GPU, t={args.t} (NC=NT={n_targets // args.batch}), "
                                  "fwd + masked CE + bwd + AdamW" + ((f" + {'all-to-all (fp32 sum at the owner)' if (reducer.wire == 'bf16' and reducer.exchange == 'a2a') else 'reduce-scatter'} / sharded AdamW / all-gather ({reducer.wire} wire)" if reducer.mode == "sharded" else " + bucketed fp32 all-reduce") if reducer.active else ""),
                      "global_batch": args.batch * world, "parallelism": f"dp{world}", "dropout": args.dropout,
                      "optimizer": "in-backward (fused into the weight-gradient launches)" if loop.fused_optimizer else
                                   ("sharded over ranks" if reducer.active and reducer.mode == "sharded" else
                                    "replicated, behind a bucketed fp32 all-reduce" if reducer.active else "separate"),
                      "loss": round(float(stats[4]), 4)}}
    if not args.full:
        out["data_parallel"] = {"dp_mode": reducer.mode, "wire": reducer.wire if reducer.mode == "sharded" else "fp32", "backend": backend,
                                "dp_fallback": dp_fallback, "bytes_on_wire_per_step": int(wire_bytes_per_step)} if reducer.active else None
        if rank == 0:
            os.write(real_stdout, (json.dumps(out) + "\n").encode())
        if world > 1 or dp_force:
            dist.barrier()
            dist.destroy_process_group()
        return

    # --full: more windows of the same length behind it (outside the judged region): their spread says how much of a difference
    # between two runs of this line is the box and how much the code
    # the extra windows also carry a one-wave clock probe on a second stream (mebt_debug_clock_probe: shader-clock ticks per 100 MHz
    # reference tick over ~70 % of the window): the clock the chip really runs this step at - the judged window stays untouched
    extra, clock_ghz = [], []
    probe_stream = None
    if rank == 0:       # a stream on ANOTHER hardware queue than the compute stream (two streams of one queue run in submission order: the steps
        from mebt_amd.parallel import pick_concurrent_stream, streams_serialised     # would wait for the sleeping probe)
        probe_stream = pick_concurrent_stream(torch.cuda.current_stream(), device=device)
        if streams_serialised(probe_stream, torch.cuda.current_stream()):
            probe_stream = None
    for _ in range(max(0, args.windows - 1)):
        buf = None
        if probe_stream is not None:
            buf = torch.zeros(4, dtype=torch.int64, device=device)
            torch.cuda.synchronize()
            try:        # diagnostics must never cost the line: at most 0.9 s of the window (the probe refuses more than one second)
                _lib.check(_lib.load().mebt_debug_clock_probe(_lib.ptr(buf), min(int(0.7 * elapsed * 1e8), 90_000_000), probe_stream.cuda_stream))
            except Exception as e:          # noqa: BLE001
                print(f"[bench] clock probe skipped: {e}", file=sys.stderr, flush=True)
                buf = None
        extra.append(window()[0])
        if buf is not None:
            torch.cuda.synchronize()
            t0_, r0_, t1_, r1_ = (int(v) for v in buf.cpu().tolist())
            if r1_ > r0_:
                clock_ghz.append(round((t1_ - t0_) / (r1_ - r0_) * 0.1, 3))
    if sampler is not None:
        sampler.__exit__()
    gpu_after = gpu_state(local_rank) if rank == 0 else None
    win_ms = [round(1e3 * e / args.steps, 3) for e in [elapsed] + extra]
    # host side of a step: wall time of two step() calls that only enqueue (empty queue in front, no synchronisation inside)
    sync()
    h0 = time.perf_counter()
    for _ in range(2):
        loop.step(x, idx, t=args.t)
    host_enqueue_ms = 1e3 * (time.perf_counter() - h0) / 2
    sync()

    # dominant kernel family: MFMA GEMMs — time every launch of 2 more steps with HIP events on the
    # launch stream (rank 0 records; every rank runs the steps because they contain collectives).  Taken BEFORE the
    # data-parallel self-description below, whose elided / one-rank steps leave the ranks' weights inconsistent
    lib = _lib.load()
    if rank == 0:
        lib.mebt_profile_enable(1)
    for _ in range(2):
        loop.step(x, idx, t=args.t)
    sync()
    roof = None
    fw_waits = None
    n, tms, fl = C.c_double(), C.c_double(), C.c_double()
    if rank == 0 and reducer.active:
        cap = 256
        wl, wm = (C.c_int32 * cap)(), (C.c_double * cap)()
        k = lib.mebt_profile_read_waits(cap, wl, wm)
        if k > 0:      # per bucket (keyed by the first layer that reads it: -1 = embeddings / biases / LayerNorms, n_layer = head): ms per step
            acc = {}
            for i in range(min(k, cap)):
                acc[int(wl[i])] = acc.get(int(wl[i]), 0.0) + float(wm[i])
            fw_waits = {str(key): round(v / 2, 4) for key, v in sorted(acc.items())}
    if rank == 0:
        _lib.check(lib.mebt_profile_read(0, C.byref(n), C.byref(tms), C.byref(fl)))
        nb, tb, by = C.c_double(), C.c_double(), C.c_double()
        _lib.check(lib.mebt_profile_read(1, C.byref(nb), C.byref(tb), C.byref(by)))
        lib.mebt_profile_enable(0)
        peak = PEAK_BF16_TFLOPS if args.dtype == "bf16" else PEAK_F32_TFLOPS
        # HBM-side bytes per GEMM launch from the committed rocprofv3 PMC passes of this same command (separate
        # FETCH_SIZE / WRITE_SIZE passes, gfx950 x2 read correction: tools/pmc_traffic.py).  PMC counters cannot be
        # collected inside this process; the source file is named so that a stale figure is visible.
        traffic, traffic_src, traffic_stale = None, None, None
        if args.dtype == "bf16" and world == 1:
            from mebt_amd.launch import csrc_fingerprint
            for fn in TRAFFIC_FILES:
                try:
                    with open(os.path.join(ROOT, "profiles", fn)) as f:
                        prof = json.load(f)
                    traffic = round(prof["gemm_bf16"]["hbm_bytes_per_launch"])
                    traffic_src = "profiles/" + fn
                    # a PMC profile belongs to the kernel sources it was taken on: anything else is reported as stale, not as a number
                    traffic_stale = prof.get("_csrc_sha256") != csrc_fingerprint()
                    if traffic_stale:
                        traffic = None
                    break
                except (OSError, KeyError, ValueError):
                    continue
        achieved = fl.value / (tms.value * 1e-3) / 1e12 if tms.value > 0 else 0.0
        roof = {"bound": "mfma", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_source": traffic_src, "traffic_stale": traffic_stale,
                "algorithmic_bytes_per_launch": round(by.value / max(1.0, nb.value)),
                "kernel": "bf16 MFMA GEMM family (gemm_bf16_dma[_ks2] / gemm_pair / wgrad_grouped incl. its fused AdamW epilogue)" if args.dtype == "bf16" else "gemm_f32_kernel",
                "launches_per_step": n.value / 2, "gemm_ms_per_step": round(tms.value / 2, 3),
                "gemm_gflop_per_step": round(fl.value / 2 / 1e9, 1)}

    # data-parallel runs describe themselves: which path ran, how many ranks RCCL really spans, what went
    # over the wire, how much of the communication was NOT hidden, and the efficiency against this same GPU's one-rank step
    dp = None
    if reducer.active:
        ones = torch.ones(1, device=device)
        dist.all_reduce(ones)
        K = max(4, min(10, args.steps))

        def timed_steps(lp, n):
            for _ in range(2):
                lp.step(x, idx, t=args.t)
            sync()
            t1 = time.perf_counter()
            for _ in range(n):
                lp.step(x, idx, t=args.t)
            sync()
            el = time.perf_counter() - t1
            if world > 1:
                tt = torch.tensor([el], device=device, dtype=torch.float64)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                el = float(tt.item())
            return 1e3 * el / n

        # (a) the same step with every collective elided (local copies / no-ops, same kernels and stream hand-offs)
        reducer.elide = True
        nocomm_ms = timed_steps(loop, K)
        reducer.elide = False
        reducer.finish()
        # (b) this GPU alone: gradients stored + separate AdamW (what a rank computes, minus the sharding), and the fused
        # single-GPU step the N = 1 headline runs — every rank measures its own, no collectives inside
        torch.cuda.synchronize()
        solo = {}
        for name, fused in (("separate_optimizer", False), ("fused_optimizer", True)):
            lp = TrainLoop(model, GradReducer(world_size=1, force=False), fused_optimizer=fused)
            lp.step_count = loop.step_count
            for _ in range(2):
                lp.step(x, idx, t=args.t)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(K):
                lp.step(x, idx, t=args.t)
            torch.cuda.synchronize()
            solo[name] = 1e3 * (time.perf_counter() - t1) / K
        model._reducer = reducer
        loop.native.enable_wire_grads(loop.wire_grads)       # the one-rank loops above unbound it
        # the two ways to exchange a bf16 bucket, timed on this node (a 4-layer bucket: 50.3 M gradients = 100.7 MB per rank): the default
        # all-to-all (fp32 sum at the owner) against RCCL's reduce-scatter (bf16 sum) - MEBT_DP_EXCHANGE picks; max over ranks, median of 5
        exchange_probe = None
        if backend == "nccl":
            try:
                nb = 4 * 12 * 1024 * 1024
                nb -= nb % (4 * world)
                send = torch.zeros(nb, dtype=torch.bfloat16, device=device)
                recv = torch.empty(nb, dtype=torch.bfloat16, device=device)
                shard = torch.empty(nb // world, dtype=torch.bfloat16, device=device)
                exchange_probe = {}
                for name, fn in (("all_to_all_ms", lambda: dist.all_to_all_single(recv, send)),
                                 ("reduce_scatter_ms", lambda: dist.reduce_scatter_tensor(shard, send, op=dist.ReduceOp.SUM))):
                    ts_ = []
                    for it in range(7):
                        sync()
                        t1 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        el = time.perf_counter() - t1
                        if world > 1:
                            tt = torch.tensor([el], device=device, dtype=torch.float64)
                            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                            el = float(tt.item())
                        if it >= 2:
                            ts_.append(1e3 * el)
                    exchange_probe[name] = round(sorted(ts_)[len(ts_) // 2], 3)
                exchange_probe["bucket_MB"] = round(nb * 2 / 1e6, 1)
                del send, recv, shard
            except Exception as e:          # noqa: BLE001
                exchange_probe = {"error": f"{type(e).__name__}: {e}"}
        dp = {"dp_mode": reducer.mode, "wire": reducer.wire if reducer.mode == "sharded" else "fp32",
              "gradient_sum": ("fp32 at the owning rank (bf16 all-to-all of the shards, mebt_adamw_slice_pieces)" if (reducer.mode == "sharded" and reducer.wire == "bf16" and reducer.exchange == "a2a")
                               else "bf16 inside RCCL's reduce-scatter" if (reducer.mode == "sharded" and reducer.wire == "bf16") else "fp32 inside RCCL"),
              "rccl_ranks": int(ones.item()), "backend": backend, "dp_fallback": dp_fallback,
              "deferred_gathers": bool(reducer.defer), "buckets": reducer.bucket_plan(loop.native.n_layer),
              "bytes_on_wire_per_step": int(wire_bytes_per_step),
              "step_ms_collectives_elided": round(nocomm_ms, 3),
              "exposed_comm_ms": round(ms - nocomm_ms, 3),
              "exposed_comm_method": "timed step minus the same step with every collective replaced by a local copy / no-op (max over ranks, same barrier-bracketed timer)",
              "exposed_forward_wait_ms_per_bucket": fw_waits,
              "exposed_forward_wait_note": "event pairs around the next forward's waits for the deferred all-gathers (two profiled steps, ms per step), "
                                           "keyed by the first block that reads the bucket (-1: non-Linear parameters, n_layer: head)",
              "one_rank_ms": {k: round(v, 3) for k, v in solo.items()},
              "scaling_efficiency": round(solo["fused_optimizer"] / ms, 4),
              "scaling_efficiency_vs_separate_optimizer": round(solo["separate_optimizer"] / ms, 4),
              "scaling_efficiency_note": "per-GPU throughput of this run / per-GPU throughput of ONE rank of this job alone on its GPU (rank 0's figure): "
                                         "against the fused step the N = 1 headline runs (the judged figure), and against gradients stored + streaming AdamW "
                                         "(what a rank computes, minus the sharding)",
              "exchange_probe": exchange_probe,
              "gemm_table_sync": "one broadcast of rank 0's GEMM tuning table behind the warm-up; further syncs (a host read that drains every rank's "
                                 "queue; every 256 steps in training) are HELD while the windows are timed",
              "comm_env": comm_env()}

    if rank == 0:
        out.update({"host_enqueue_ms_per_step": round(host_enqueue_ms, 3),
                    "windows": {"ms_per_step": win_ms, "median": sorted(win_ms)[len(win_ms) // 2], "min": min(win_ms), "max": max(win_ms),
                                "note": f"{len(win_ms)} back-to-back windows of {args.steps} steps, each barrier + synchronize bracketed; `value` is the FIRST"},
                    "gpu_state": {"before": gpu_before, "after": gpu_after, "during_windows": sampler.summary() if sampler is not None else None,
                                  "shader_clock_ghz_in_extra_windows": clock_ghz,
                                  "note": "amdgpu sysfs: current sclk / mclk / fclk level, power cap / average before and after the windows (idle readings), "
                                          "and sclk / power sampled every 25 ms by a host thread while they run (the sysfs sclk need not follow the load: "
                                          "`shader_clock_ghz_in_extra_windows` is measured in a kernel, s_memtime against the 100 MHz s_memrealtime, beside the steps of the "
                                          "windows behind the judged one)"},
                    "roofline": roof, "data_parallel": dp})
        # the legs below run outside the timed region; a failure in one of them must not cost the headline line
        if world == 1 and args.secondary != "none" and args.preset == "sky_16f":
            try:
                out["secondary"] = secondary_metrics(args, cfg, model, loop, x, idx, device, lib, args.secondary)
            except Exception as e:          # noqa: BLE001
                out["secondary"] = {"error": f"{type(e).__name__}: {e}"}
        if not args.no_cpu_baseline and world == 1:
            try:
                sd = {k: v.detach() for k, v in model.state_dict().items()}
                out["cpu_baseline"] = cpu_baseline(sd, cfg, args.t)
            except Exception as e:          # noqa: BLE001
                out["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if world > 1 or dp_force:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
