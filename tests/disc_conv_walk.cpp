// Walks mebt_amd/csrc/disc/disc_addr.h on the CPU the way the kernels of csrc/disc/disc_conv.hip use it: for every workgroup of the
// grid, every one of its 256 threads and every K slice, serially.  Built and run by tests/test_host_disc_conv.py with the system
// compiler; no HIP.  Per case it allocates input, weight, output and slot buffers of exactly the element counts the Python side
// allocates and checks by its own comparisons that every read and write lies inside its buffer and is aligned to its vector width,
// that every output element and every slot is written exactly once, that no row at or past M and no column at or past Cout
// contributes, and that the convolution computed through these functions on small integer data equals a direct seven-loop
// convolution exactly.  Exit status 0 and a last line "ok: <cases> cases" when every case holds.
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../mebt_amd/csrc/disc/disc_addr.h"

namespace {

int failures = 0;
std::string current;

void fail(const char* what, long a = 0, long b = 0, long c = 0) {
    if (++failures <= 30) printf("FAIL %s: %s (%ld, %ld, %ld)\n", current.c_str(), what, a, b, c);
}

// small integers, never all zero along a row
int in_value(int64_t i) { return (int)((i * 7 + i / 13 + 3) % 7) - 3; }
int w_value(int64_t i) { return (int)((i * 5 + i / 11 + 1) % 5) - 2; }
int bias_value(int n) { return n % 9 - 4; }

struct Stage { int B, Ti, Hi, Wi, Cin, kt, stride, Cout; bool head, slots; };

// logical weight [Cout][Cin][kt][4][4] -> [Npad][Kpad], K order (tap, ci), zeros in the padding: what arrange_weight does
std::vector<int> arrange(const DiscGeom& g, const std::vector<int>& w) {
    std::vector<int> a((size_t)disc_w_elems(g), 0);
    for (int n = 0; n < g.Cout; ++n)
        for (int ci = 0; ci < g.Cin; ++ci)
            for (int tap = 0; tap < g.kt * 16; ++tap)
                a[(size_t)n * g.Kpad + (size_t)tap * g.Cin + ci] = w[((size_t)n * g.Cin + ci) * g.kt * 16 + tap];
    return a;
}

// the seven loops: b, to, ho, wo, n, tap, ci
std::vector<long> direct(const DiscGeom& g, const std::vector<int>& in, const std::vector<int>& w) {
    std::vector<long> out((size_t)disc_out_elems(g), 0);
    for (int b = 0; b < g.B; ++b)
        for (int to = 0; to < g.To; ++to)
            for (int ho = 0; ho < g.Ho; ++ho)
                for (int wo = 0; wo < g.Wo; ++wo) {
                    const size_t m = (((size_t)b * g.To + to) * g.Ho + ho) * g.Wo + wo;
                    for (int n = 0; n < g.Cout; ++n) {
                        long s = bias_value(n);
                        for (int tap = 0; tap < g.kt * 16; ++tap) {
                            const int dt = tap / 16, dh = tap / 4 % 4, dw = tap % 4;
                            const int ti = g.kt == 4 ? to * g.stride - 2 + dt : 0, hi = ho * g.stride - 2 + dh, wi = wo * g.stride - 2 + dw;
                            if (ti < 0 || ti >= g.Ti || hi < 0 || hi >= g.Hi || wi < 0 || wi >= g.Wi) continue;
                            const int* x = &in[((((size_t)b * g.Ti + ti) * g.Hi + hi) * g.Wi + wi) * g.Cin];
                            const int* wr = &w[(size_t)n * g.Cin * g.kt * 16 + tap];
                            for (int ci = 0; ci < g.Cin; ++ci) s += (long)x[ci] * wr[(size_t)ci * g.kt * 16];
                        }
                        out[m * g.Cout + n] = s;
                    }
                }
    return out;
}

struct Buffers {
    DiscGeom g;
    std::vector<int> in, wl, wa;
    std::vector<long> out, want;
    std::vector<int> out_writes;
};

Buffers make(const Stage& s, int eb) {
    Buffers u;
    u.g = disc_geom(s.B, s.Ti, s.Hi, s.Wi, s.Cin, s.kt, s.stride, s.Cout, eb);
    const DiscGeom& g = u.g;
    u.in.resize((size_t)disc_in_elems(g));
    for (size_t i = 0; i < u.in.size(); ++i) u.in[i] = (g.Cin == 4 && i % 4 == 3) ? 0 : in_value((int64_t)i);     // the zero fourth channel
    u.wl.resize((size_t)g.Cout * g.Cin * g.kt * 16);
    for (size_t i = 0; i < u.wl.size(); ++i) u.wl[i] = w_value((int64_t)i);
    u.wa = arrange(g, u.wl);
    u.out.assign((size_t)disc_out_elems(g), -777777);
    u.out_writes.assign(u.out.size(), 0);
    u.want = direct(g, u.in, u.wl);
    return u;
}

void check_read(const char* what, int64_t off, int n, int64_t elems) {
    if (off < 0 || off + n > elems) fail(what, off, n, elems);
    if (off % n) fail("misaligned", off, n);
}

void compare(const Buffers& u) {
    for (size_t i = 0; i < u.out.size(); ++i) {
        if (u.out_writes[i] != 1) { fail("an output element not written exactly once", (long)i, u.out_writes[i]); break; }
        if (u.out[i] != u.want[i]) { fail("differs from the direct convolution", (long)i, u.out[i], u.want[i]); break; }
    }
}

void walk_conv(const Stage& s, int eb) {
    Buffers u = make(s, eb);
    const DiscGeom& g = u.g;
    const int BM = g.BM, VEC = g.VEC, SUB = g.VEC / g.GV, WM = BM / 64;
    const int ACH = BM * DISC_BK / VEC / DISC_THREADS, BCH = DISC_BN * DISC_BK / VEC / DISC_THREADS;
    const int64_t M = disc_rows(g), tiles = disc_row_tiles(g);
    if (disc_K(g) > g.Kpad || g.Kpad % DISC_BK || g.Npad % DISC_BN || g.Npad < g.Cout) fail("padding", g.Kpad, g.Npad);
    if (g.GV * SUB != VEC || g.Cin % g.GV) fail("vector width", g.GV, VEC, g.Cin);
    if (g.cin_shift >= 0 ? g.Cin != 1 << g.cin_shift : (g.Cin & (g.Cin - 1)) == 0) fail("cin_shift", g.Cin, g.cin_shift);
    std::vector<double> slots(s.slots ? (size_t)disc_slot_count(g) : 0, 0.0);
    std::vector<int> slot_writes(slots.size(), 0);
    std::vector<int> sA((size_t)BM * DISC_BK), sB((size_t)DISC_BN * DISC_BK), wrA(sA.size()), wrB(sB.size());
    std::vector<long> acc((size_t)BM * DISC_BN);
    std::vector<int> cover(acc.size());

    for (int64_t bx = 0; bx < tiles; ++bx)
        for (int by = 0; by < g.Npad / DISC_BN; ++by) {
            const int64_t m0 = bx * BM;
            const int n0 = by * DISC_BN;
            std::fill(acc.begin(), acc.end(), 0L);
            for (int kk = 0; kk < g.Kpad / DISC_BK; ++kk) {
                const int kb = kk * DISC_BK;
                std::fill(wrA.begin(), wrA.end(), 0);
                std::fill(wrB.begin(), wrB.end(), 0);
                for (int tid = 0; tid < DISC_THREADS; ++tid) {
                    for (int i = 0; i < ACH; ++i) {
                        const DiscChunk c = disc_stage_chunk(tid, i, VEC);
                        if (c.row < 0 || c.row >= BM || c.ch < 0 || c.ch >= DISC_BK / VEC) { fail("A chunk outside the tile", c.row, c.ch); continue; }
                        const DiscOrg org = disc_row_origin(g, m0 + c.row);
                        if ((org.ok != 0) != (m0 + c.row < M)) fail("row origin: ok", m0 + c.row, org.ok);
                        for (int sub = 0; sub < SUB; ++sub) {
                            const int k = kb + c.ch * VEC + sub * g.GV;
                            int64_t off = -1;
                            const bool reads = disc_in_offset(g, org, k, off);
                            if (reads && (m0 + c.row >= M || k >= disc_K(g))) fail("a row past M or a k past K reads", m0 + c.row, k);
                            if (reads) check_read("input read outside the buffer", off, g.GV, disc_in_elems(g));
                            for (int e = 0; e < g.GV; ++e) {
                                const size_t at = (size_t)c.row * DISC_BK + c.ch * VEC + sub * g.GV + e;
                                sA[at] = reads && off >= 0 && off + g.GV <= disc_in_elems(g) ? u.in[(size_t)off + e] : 0;
                                ++wrA[at];
                            }
                        }
                    }
                    for (int i = 0; i < BCH; ++i) {
                        const DiscChunk c = disc_stage_chunk(tid, i, VEC);
                        if (c.row < 0 || c.row >= DISC_BN || c.ch < 0 || c.ch >= DISC_BK / VEC) { fail("B chunk outside the tile", c.row, c.ch); continue; }
                        const int64_t off = disc_w_offset(g, n0 + c.row, kb + c.ch * VEC);
                        check_read("weight read outside the buffer", off, VEC, disc_w_elems(g));
                        for (int e = 0; e < VEC; ++e) {
                            const size_t at = (size_t)c.row * DISC_BK + c.ch * VEC + e;
                            sB[at] = off >= 0 && off + VEC <= disc_w_elems(g) ? u.wa[(size_t)off + e] : 0;
                            ++wrB[at];
                        }
                    }
                }
                for (size_t i = 0; i < wrA.size(); ++i) if (wrA[i] != 1) { fail("an A cell not staged exactly once", (long)i, wrA[i]); break; }
                for (size_t i = 0; i < wrB.size(); ++i) if (wrB[i] != 1) { fail("a B cell not staged exactly once", (long)i, wrB[i]); break; }
                for (int r = 0; r < BM; ++r)
                    for (int c = 0; c < DISC_BN; ++c) {
                        long t = 0;
                        for (int k = 0; k < DISC_BK; ++k) t += sA[(size_t)r * DISC_BK + k] * sB[(size_t)c * DISC_BK + k];
                        acc[(size_t)r * DISC_BN + c] += t;
                    }
            }
            // the epilogue through the fragment map
            std::fill(cover.begin(), cover.end(), 0);
            std::vector<double> s1(DISC_BN, 0.0), s2(DISC_BN, 0.0);
            for (int wave = 0; wave < 4; ++wave)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < WM; ++i)
                        for (int j = 0; j < 4; ++j)
                            for (int r = 0; r < 4; ++r) {
                                const int row = disc_frag_row(wave, i, lane, WM), col = disc_frag_col(j, lane, r);
                                if (row < 0 || row >= BM || col < 0 || col >= DISC_BN) { fail("fragment outside the tile", row, col); continue; }
                                ++cover[(size_t)row * DISC_BN + col];
                                const int64_t m = m0 + row;
                                const int n = n0 + col;
                                const long v = acc[(size_t)row * DISC_BN + col] + (n < g.Cout ? bias_value(n) : 0);
                                if (m < M) { s1[col] += (double)v; s2[col] += (double)v * (double)v; }
                                int64_t off = -1;
                                const bool stores = disc_out_offset(g, m, n, off);
                                if (stores != (m < M && n < g.Cout)) fail("a row past M or a column past Cout stores (or one inside does not)", m, n);
                                if (!stores) continue;
                                if (off < 0 || off >= disc_out_elems(g)) { fail("output write outside the buffer", off, m, n); continue; }
                                u.out[(size_t)off] = v;
                                ++u.out_writes[(size_t)off];
                            }
            for (size_t i = 0; i < cover.size(); ++i) if (cover[i] != 1) { fail("a tile element not held exactly once", (long)i, cover[i]); break; }
            if (s.slots)
                for (int tid = 0; tid < 2 * DISC_BN; ++tid) {
                    const int q = tid >> 6, col = tid & 63;
                    int64_t off = -1;
                    const bool stores = disc_slot_offset(g, n0 + col, q, bx, off);
                    if (stores != (n0 + col < g.Cout)) fail("a column past Cout has a slot (or one inside has none)", n0 + col, q);
                    if (!stores) continue;
                    if (off < 0 || off >= disc_slot_count(g)) { fail("slot write outside the buffer", off, n0 + col, q); continue; }
                    slots[(size_t)off] = q ? s2[col] : s1[col];
                    ++slot_writes[(size_t)off];
                }
        }
    compare(u);
    if (s.slots) {
        // a slot holds exactly the rows of its tile: compare with sums over the direct convolution
        for (int c = 0; c < g.Cout; ++c)
            for (int q = 0; q < 2; ++q)
                for (int64_t t = 0; t < tiles; ++t) {
                    const size_t at = ((size_t)c * 2 + q) * tiles + t;
                    if (slot_writes[at] != 1) { fail("a slot not written exactly once", c, q, t); continue; }
                    double want = 0.0;
                    for (int64_t m = t * BM; m < (t + 1) * BM && m < M; ++m) {
                        const double v = (double)u.want[(size_t)m * g.Cout + c];
                        want += q ? v * v : v;
                    }
                    if (slots[at] != want) fail("slot differs from its rows' sum", c, q, t);
                }
    }
}

void walk_head(const Stage& s, int eb) {
    Buffers u = make(s, eb);
    const DiscGeom& g = u.g;
    if (g.GV != g.VEC || g.Cout != 1) { fail("the one-channel stage needs Cin a multiple of the vector", g.Cin, g.VEC); return; }
    const int64_t M = disc_rows(g), blocks = (M + 3) / 4;
    const int K = disc_K(g), iters = disc_head_iters(g);
    if (disc_head_flush_iters(g) < 1) fail("flush interval", disc_head_flush_iters(g));
    std::vector<int> seen((size_t)K / g.VEC);
    for (int64_t bx = 0; bx < blocks; ++bx)
        for (int wave = 0; wave < 4; ++wave) {
            const int64_t m = bx * 4 + wave;
            if (m >= M) continue;
            const DiscOrg org = disc_row_origin(g, m);
            std::fill(seen.begin(), seen.end(), 0);
            long acc = 0;
            for (int lane = 0; lane < 64; ++lane)
                for (int it = 0; it < iters; ++it) {
                    const int k = disc_head_k(g, it, lane);
                    if (k % g.VEC || k < 0) fail("k not a chunk", k);
                    if (k >= K) continue;
                    ++seen[(size_t)k / g.VEC];
                    int64_t off = -1;
                    if (!disc_in_offset(g, org, k, off)) continue;
                    check_read("input read outside the buffer", off, g.VEC, disc_in_elems(g));
                    const int64_t woff = disc_w_offset(g, 0, k);
                    check_read("weight read outside the buffer", woff, g.VEC, disc_w_elems(g));
                    if (off < 0 || off + g.VEC > disc_in_elems(g) || woff < 0 || woff + g.VEC > disc_w_elems(g)) continue;
                    for (int e = 0; e < g.VEC; ++e) acc += (long)u.in[(size_t)off + e] * u.wa[(size_t)woff + e];
                }
            for (size_t i = 0; i < seen.size(); ++i) if (seen[i] != 1) { fail("a chunk of K not visited exactly once", (long)i, seen[i]); break; }
            int64_t off = -1;
            if (!disc_out_offset(g, m, 0, off) || off < 0 || off >= disc_out_elems(g)) { fail("output write outside the buffer", off, m); continue; }
            u.out[(size_t)off] = acc + bias_value(0);
            ++u.out_writes[(size_t)off];
        }
    compare(u);
}

// ingest: every destination voxel's four channels written once inside [B, To, H, W, 4], every source read inside [B, 3, T, H, W]
void walk_ingest(int B, int T, int H, int W, bool frames) {
    const int To = frames ? 1 : T;
    const int64_t src = (int64_t)B * 3 * T * H * W, dst = (int64_t)B * To * H * W * 4;
    std::vector<int> writes((size_t)dst, 0), reads((size_t)src, 0);
    for (int64_t b = 0; b < B; ++b)
        for (int t = 0; t < To; ++t)
            for (int h = 0; h < H; ++h)
                for (int w = 0; w < W; ++w) {
                    const int f = frames ? (int)((b * 5 + 2) % T) : t;
                    for (int c = 0; c < 3; ++c) {
                        const int64_t off = disc_ingest_src(T, H, W, b, c, f, h, w);
                        if (off < 0 || off >= src) fail("ingest read outside the buffer", off, src);
                        else if (off != (((b * 3 + c) * T + f) * H + h) * W + w) fail("ingest source", off);
                        else ++reads[(size_t)off];
                    }
                    const int64_t off = disc_ingest_dst(To, H, W, b, t, h, w);
                    if (off < 0 || off + 4 > dst || off % 4) { fail("ingest write outside the buffer or misaligned", off, dst); continue; }
                    for (int e = 0; e < 4; ++e) ++writes[(size_t)off + e];
                }
    for (size_t i = 0; i < writes.size(); ++i) if (writes[i] != 1) { fail("an ingest element not written exactly once", (long)i, writes[i]); break; }
    if (!frames)
        for (size_t i = 0; i < reads.size(); ++i) if (reads[i] != 1) { fail("a source element not read exactly once", (long)i, reads[i]); break; }
}

int cases = 0;

void run(const std::string& name, const Stage& s) {
    for (int eb : {2, 4}) {
        current = name + (eb == 2 ? " f16" : " f32");
        if (s.head) walk_head(s, eb); else walk_conv(s, eb);
        ++cases;
    }
}

// every stage of a network (vqgan.py:423-444) on an input [B, 3 (stored 4), T, H, W]
void run_network(const std::string& name, bool three_d, int ndf, int L, int B, int T, int H, int W) {
    int cin = 4, nf = ndf, t = T, h = H, w = W;
    const int kt = three_d ? 4 : 1;
    for (int n = 0; n < L + 2; ++n) {
        const int stride = n < L ? 2 : 1;
        int cout = ndf;
        if (n >= 1 && n <= L) { nf = nf * 2 < 512 ? nf * 2 : 512; cout = nf; }
        if (n == L + 1) cout = 1;
        run(name + " stage " + std::to_string(n), Stage{B, t, h, w, cin, kt, stride, cout, n == L + 1, n >= 1 && n <= L});
        t = three_d ? disc_out_extent(t, stride) : 1;
        h = disc_out_extent(h, stride);
        w = disc_out_extent(w, stride);
        cin = cout;
    }
}

}  // namespace

int main() {
    // the five golden cases (tests/golden/disc/make_golden_disc.py CASES)
    run_network("img8", false, 8, 3, 3, 1, 20, 12);
    run_network("vid8", true, 8, 3, 2, 5, 20, 12);
    run_network("vid8t1", true, 8, 2, 2, 1, 8, 6);
    run_network("img64", false, 64, 3, 2, 1, 16, 16);
    run_network("vid64", true, 64, 3, 2, 4, 16, 16);
    // the edge shapes of tests/test_gpu_disc_forward.py
    run("stage 0 2D 5x3", Stage{2, 1, 5, 3, 4, 1, 2, 8, false, false});
    run("stage 0 3D 3x5x3", Stage{2, 3, 5, 3, 4, 4, 2, 8, false, false});
    run("8 -> 8 stride 1 2D", Stage{2, 1, 5, 3, 8, 1, 1, 8, false, true});
    run("8 -> 8 stride 2 2D", Stage{2, 1, 5, 3, 8, 1, 2, 8, false, true});
    run("8 -> 8 stride 1 3D", Stage{2, 3, 5, 3, 8, 4, 1, 8, false, true});
    run("8 -> 8 stride 2 3D", Stage{2, 3, 5, 3, 8, 4, 2, 8, false, true});
    run("8 -> 72", Stage{2, 1, 5, 3, 8, 1, 2, 72, false, true});
    run("24 -> 8 (Cin no power of two)", Stage{2, 1, 5, 3, 24, 1, 2, 8, false, true});
    run("3D with T = 1", Stage{2, 1, 5, 3, 8, 4, 2, 16, false, true});
    for (int bm : {64, 128})
        for (int d : {-1, 0, 1}) run("1x1 stride 2 B = " + std::to_string(bm + d), Stage{bm + d, 1, 1, 1, 8, 1, 2, 8, false, true});
    run("one channel K 128", Stage{3, 1, 5, 3, 8, 1, 1, 1, true, false});
    run("one channel 3D K 1536", Stage{2, 2, 3, 4, 24, 4, 1, 1, true, false});
    // ingest: clips, frames, and one frame of every clip
    current = "ingest clips"; walk_ingest(2, 5, 20, 12, false); ++cases;
    current = "ingest frames"; walk_ingest(3, 1, 20, 12, false); ++cases;
    current = "ingest frame_idx"; walk_ingest(3, 5, 7, 3, true); ++cases;
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("ok: %d cases\n", cases);
    return 0;
}
