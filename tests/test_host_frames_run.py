"""The byte-run writer and the chunk rule of the frame kernels (mebt_amd/csrc/frames/byte_run.h) walked on the CPU: the stand-alone
program tests/frames_run_walk.cpp, built with the system C++ compiler (no HIP), goes through every chunk and lane of the gather and
video kernels' uint8 path for run lengths around the chunk size, every offset from a dword boundary and 1..5 frames back to back."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_chunk_and_lane_writes_its_bytes_once(tmp_path):
    exe = str(tmp_path / "frames_run_walk")
    cc = subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "frames_run_walk.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.splitlines()[-1] == "ok: 300 cases", r.stdout[-3000:]
