// Walks mebt_amd/csrc/frames/byte_run.h on the CPU the way pack_gather_kernel<uint8_t> and video_to_clip_kernel use it: for every
// frame of a launch, every chunk k < run_chunks(...) and every one of the 256 lanes, serially.  Built and run by
// tests/test_host_frames_run.py with the system compiler; no HIP.  Exit status 0 and a last line "ok: <cases> cases" when every case holds.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../mebt_amd/csrc/frames/byte_run.h"

namespace {

constexpr int THREADS = 256;                // FR_THREADS
constexpr int GUARD = 64;
constexpr uint8_t GUARD_BYTE = 0xEE;

// never 0: a byte that no lane wrote, or that a neighbouring dword's empty lanes wrote over, shows
uint8_t expected(int frame, int j) { return (uint8_t)(1 + (frame * 131 + j * 7 + j / 251) % 255); }

int failures = 0;

void fail(const char* what, int nrun, int off, int frames, long a = 0, long b = 0) {
    if (++failures <= 20) printf("FAIL nrun=%d offset=%d frames=%d: %s (%ld, %ld)\n", nrun, off, frames, what, a, b);
}

// the chunks k < nchunk partition [0, nrun) in order and none is longer than PK_CHUNK; empty chunks (c0 >= c1) only at the end
void check_partition(long nchunk, int mis, int nrun, int off, int frames) {
    int next = 0;
    for (int k = 0; k < nchunk; ++k) {
        const RunChunk ch = run_chunk(k, mis, nrun);
        if (ch.j0 != k * PK_CHUNK - mis) fail("j0", nrun, off, frames, k, ch.j0);
        if (ch.c0 >= ch.c1) {
            if (next != nrun) fail("an empty chunk before the run's end", nrun, off, frames, k, next);
            continue;
        }
        if (ch.c0 != next) fail("chunks do not follow each other", nrun, off, frames, k, ch.c0);
        if (ch.c1 - ch.c0 > PK_CHUNK) fail("chunk longer than PK_CHUNK", nrun, off, frames, k, ch.c1 - ch.c0);
        next = ch.c1;
    }
    if (next != nrun) fail("chunks do not reach the run's end", nrun, off, frames, next, nchunk);
}

// one launch over `frames` runs back to back from a pointer `off` bytes past a dword boundary; `backwards`: the chunks of a run in
// descending order (on the device they run in any order, and none may touch a byte of another)
void walk(int nrun, int off, int frames, bool backwards) {
    const size_t total = (size_t)nrun * frames;
    std::vector<uint8_t> mem(total + 2 * GUARD + 32, GUARD_BYTE);
    uint8_t* base = mem.data();
    base += (16 - reinterpret_cast<uintptr_t>(base) % 16) % 16;
    uint8_t* out = base + GUARD + off;      // GUARD is a multiple of 4: out is `off` bytes past a dword boundary
    for (size_t i = 0; i < total; ++i) out[i] = 0;
    std::vector<int> made(total, 0);        // how often a byte's value was asked for

    const long nchunk = run_chunks(nrun, out);
    for (int n = 0; n < frames; ++n) {
        uint8_t* run = out + (size_t)n * nrun;
        const int mis = run_mis(run);
        if (mis != (int)((off + (size_t)n * nrun) % 4)) fail("run_mis", nrun, off, frames, n, mis);
        check_partition(nchunk, mis, nrun, off, frames);
        int* count = made.data() + (size_t)n * nrun;
        auto byte = [&](int j) {
            if (j < 0 || j >= nrun) fail("byte outside the run", nrun, off, frames, n, j);
            else ++count[j];
            return expected(n, j);
        };
        auto quad = [&](int j, uint32_t& v) {
            if (reinterpret_cast<uintptr_t>(run + j) % 4) fail("quad off a dword boundary", nrun, off, frames, n, j);
            if (j / 4 % 3 == 0) return false;   // every third dword refused, as the resize writer does at a row boundary
            v = (uint32_t)byte(j) | (uint32_t)byte(j + 1) << 8 | (uint32_t)byte(j + 2) << 16 | (uint32_t)byte(j + 3) << 24;
            return true;
        };
        for (long i = 0; i < nchunk; ++i) {
            const int k = (int)(backwards ? nchunk - 1 - i : i);
            const RunChunk ch = run_chunk(k, mis, nrun);
            if (ch.c0 >= ch.c1) continue;   // the kernels return here
            for (int tid = 0; tid < THREADS; ++tid) write_run(run, nrun, ch.c0, ch.c1, ch.j0 + 4 * tid, 4 * THREADS, quad, byte);
        }
    }
    for (int n = 0; n < frames; ++n)
        for (int j = 0; j < nrun; ++j) {
            const size_t i = (size_t)n * nrun + j;
            if (made[i] != 1) fail("byte not made exactly once", nrun, off, frames, (long)i, made[i]);
            if (out[i] != expected(n, j)) fail("byte holds another value", nrun, off, frames, (long)i, out[i]);
        }
    for (int g = 0; g < GUARD; ++g)
        if (out[-1 - g] != GUARD_BYTE || out[total + g] != GUARD_BYTE) fail("guard band written", nrun, off, frames, g);
}

}  // namespace

int main() {
    const int nruns[] = {1, 2, 3, 5, 27, 867, 2883, 6141, 6143, 6144, 6145, 6147, 12288, 12289, 12675};
    int cases = 0;
    for (int nrun : nruns) {
        // the float gather counts its chunks from the frame's first byte
        check_partition(run_chunks(nrun, nullptr), 0, nrun, -1, 0);
        for (int off = 0; off < 4; ++off)
            for (int frames = 1; frames <= 5; ++frames, ++cases) {
                walk(nrun, off, frames, false);
                walk(nrun, off, frames, true);
            }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok: %d cases\n", cases);
    return 0;
}
