"""The engine's routing table (mebt_amd/csrc/route.h) on the CPU.  tests/engine_route_walk.cpp, built with the system C++ compiler (no
HIP), compares what the table yields with the five block modes written out by hand: shapes and the LN1 job lists of forward and
backward for every mode over NS in {0, 8, 256} x NC in {0, 5, 7936} x NT in {1, 7, 256}, and liveness / tok_live / has_maskgit for
every mode list of length 1..6 and the shipped 24-block list.  The workspace the engine carves from it is compared, byte count by byte
count, with tests/golden/workspace_bytes.json, recorded before the table existed."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def test_routes_equal_the_modes_written_out_by_hand(tmp_path):
    exe = str(tmp_path / "engine_route_walk")
    cc = subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "engine_route_walk.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.splitlines()[-1] == "ok: 19630 cases", r.stdout[-3000:]     # 99 blocks + 19 530 mode lists + the shipped list


def test_workspace_layout_is_the_recorded_one():
    """mebt_workspace_bytes / mebt_kvcache_bytes of a host-only handle (fresh process, no GPU, tuning off: the flush buffer and the
    attention keep bits change the layout) against the fixture."""
    env = {k: v for k, v in os.environ.items() if k not in ("MEBT_ATTN_DROP_BITS", "MEBT_GEMM_TUNE_FLUSH_MB")}
    env.update(MEBT_HOST_ONLY="1", MEBT_GEMM_AUTOTUNE="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "workspace_bytes_driver.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    got = json.loads(r.stdout)
    with open(os.path.join(HERE, "golden", "workspace_bytes.json")) as f:
        want = json.load(f)
    assert len(want["workspace"]) == 7 * 2 * 3 * 5 * 2 and len(want["kvcache"]) == 7 * 2
    assert all(v > 0 for v in want["workspace"].values())
    assert got == want, [(k, want["workspace"][k], got["workspace"].get(k)) for k in want["workspace"] if got["workspace"].get(k) != want["workspace"][k]][:10]
