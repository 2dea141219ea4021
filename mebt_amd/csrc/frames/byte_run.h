// Writing a run of output bytes a dword per lane (csrc/frames/frames.hip: the uint8 outputs of the resize, copy, gather and video
// kernels).  A run is nrun contiguous bytes from any address; its dwords are counted from the dword boundary at or below its start,
// `mis` bytes early: every lane stores aligned dwords and only the two ragged ends are byte stores.  The gather and video kernels
// also cut a run into chunks of PK_CHUNK bytes counted from that boundary, one workgroup each.  Plain C++ with no HIP in it:
// tests/frames_run_walk.cpp walks these functions on the CPU over every alignment.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BYTE_RUN_FN __host__ __device__ __forceinline__
#else
#define BYTE_RUN_FN inline
#endif

constexpr int PK_CHUNK = 6144;              // 2048 pixels, or 1536 dwords of the uint8 run; a multiple of 3, 4 and 16

// the bytes of `v` (lowest first) belong at run[j, j + 4), of which [0, n) exists; run + j is dword aligned
BYTE_RUN_FN void store_quad(uint8_t* run, int j, int n, uint32_t v) {
    if (j >= 0 && j + 4 <= n) {
        *reinterpret_cast<uint32_t*>(run + j) = v;
        return;
    }
    for (int c = 0; c < 4; ++c)
        if (j + c >= 0 && j + c < n) run[j + c] = (uint8_t)(v >> (8 * c));
}

// the run's offset from the dword boundary at or below it
BYTE_RUN_FN int run_mis(const uint8_t* run) { return (int)(reinterpret_cast<uintptr_t>(run) & 3); }

// chunk k of a run: its bytes are [c0, c1) of the run (none when c0 >= c1) and its first dword is at run + j0, which may lie below c0
struct RunChunk { int c0, c1, j0; };

BYTE_RUN_FN RunChunk run_chunk(int k, int mis, int nrun) {
    const int j0 = k * PK_CHUNK - mis;
    return {j0 > 0 ? j0 : 0, j0 + PK_CHUNK < nrun ? j0 + PK_CHUNK : nrun, j0};
}

// host: chunks per run of a launch whose runs of nrun bytes lie back to back from `out`.  A run starts up to `slack` bytes after the
// dword boundary its chunks are counted from: every run shares out's offset when a run is a whole number of dwords, else any offset
// occurs.  out == nullptr: the output is no byte run (the float planes) and the chunks are counted from the frame's first byte.
inline long run_chunks(long nrun, const void* out) {
    const long slack = !out ? 0 : (nrun % 4 ? 3 : (long)(reinterpret_cast<uintptr_t>(out) & 3));
    return (nrun + slack + PK_CHUNK - 1) / PK_CHUNK;
}

// Write bytes [lo, hi) of `run` (nrun bytes), this lane's dwords being those at j0, j0 + step, ... (run + j0 dword aligned, step a
// multiple of 4).  A dword that lies whole inside [lo, hi) is `quad(j, v)`'s, which sets v and returns true, or returns false with v
// untouched; any other dword, a ragged end or one that `quad` refused, is put together from `byte(jj)` of its bytes inside [lo, hi).
template <typename Quad, typename Byte>
BYTE_RUN_FN void write_run(uint8_t* run, int nrun, int lo, int hi, int j0, int step, Quad quad, Byte byte) {
    for (int j = j0; j < hi; j += step) {
        uint32_t v = 0;
        if (!(lo <= j && j + 4 <= hi && quad(j, v))) {
            for (int c = 0; c < 4; ++c)
                if (j + c >= lo && j + c < hi) v |= (uint32_t)byte(j + c) << (8 * c);
        }
        store_quad(run, j, nrun, v);
    }
}

// the same for a writer whose whole dwords are just their four bytes
template <typename Byte>
BYTE_RUN_FN void write_run(uint8_t* run, int nrun, int lo, int hi, int j0, int step, Byte byte) {
    write_run(run, nrun, lo, hi, j0, step, [&](int j, uint32_t& v) {
        v = (uint32_t)byte(j) | (uint32_t)byte(j + 1) << 8 | (uint32_t)byte(j + 2) << 16 | (uint32_t)byte(j + 3) << 24;
        return true;
    }, byte);
}
