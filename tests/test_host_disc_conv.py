"""The addressing of the discriminators' forward kernels (mebt_amd/csrc/disc/disc_addr.h) walked on the CPU: the stand-alone program
tests/disc_conv_walk.cpp, built with the system C++ compiler (no HIP), goes through every workgroup, thread and K slice of every stage
of the five golden cases, the edge shapes of tests/test_gpu_disc_forward.py and both dtypes' tiles, and checks bounds, alignment, single
writes, the exclusion of rows past M and columns past Cout, and the convolution itself against a direct seven-loop one."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_workgroup_thread_and_slice_stays_inside_its_buffers(tmp_path):
    exe = str(tmp_path / "disc_conv_walk")
    cc = subprocess.run(["c++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(HERE, "disc_conv_walk.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.splitlines()[-1] == "ok: 85 cases", r.stdout[-3000:]
