// Compares what mebt_amd/csrc/route.h derives from its routing table with the five block modes written out case by case, the way
// engine.cpp sequenced them before the table existed: attention shape, fused-vs-separate projections, the streams a block rewrites,
// the LN1 jobs of forward and backward, and which blocks the loss reaches.  Built and run by tests/test_host_engine_route.py with the
// system compiler; no HIP.  Exit status 0 and a last line "ok: <cases> cases" when every case holds.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../mebt_amd/csrc/route.h"

namespace {

enum { ENC = MEBT_MODE_LATENT_ENC, SELF = MEBT_MODE_LATENT_SELF, DEC = MEBT_MODE_LATENT_DEC, LT2L = MEBT_MODE_LT2L, MG = MEBT_MODE_MASKGIT };
const char* const NAMES[5] = {"latent_enc", "latent_self", "latent_dec", "lt2l", "maskgit"};

int failures = 0;

void fail(const char* what, int mode, int NS, int NC, int NT, long a = 0, long b = 0) {
    if (++failures <= 20) printf("FAIL %s NS=%d NC=%d NT=%d: %s (%ld, %ld)\n", mode >= 0 ? NAMES[mode] : "modes", NS, NC, NT, what, a, b);
}

// one LN1 job as the hand-written cases name it
struct Job {
    int stream, len;
    bool key;                 // forward: written to the key buffer; backward: dy = the key side's gradient, key statistics
    int seg, stride, off;
    bool add_q, key_only;     // backward: dy2 = the query side's gradient; accumulate when the stream gradient is defined
};

struct Expect {
    int NQ, NK;
    bool fused;               // one QKV product on LN1(query)
    int nout, out[2];         // the streams the block output replaces
    std::vector<Job> fwd, bwd;
};

Expect by_hand(int mode, int NS, int NC, int NT) {
    Expect e;
    switch (mode) {
        case ENC:
            e = {NS, NC, false, 1, {RT_S, RT_NONE}, {}, {}};
            e.fwd = {{RT_S, NS, false, 0, 0, 0, false, false}, {RT_C, NC, true, 0, 0, 0, false, false}};
            e.bwd = {{RT_S, NS, false, 0, 0, 0, false, false}};
            if (NC > 0) e.bwd.push_back({RT_C, NC, true, 0, 0, 0, false, true});       // contexts feed every latent_enc block
            break;
        case SELF:
            e = {NS, NS, true, 1, {RT_S, RT_NONE}, {}, {}};
            e.fwd = {{RT_S, NS, false, 0, 0, 0, false, false}};
            e.bwd = {{RT_S, NS, false, 0, 0, 0, false, false}};
            break;
        case DEC:
            e = {NT, NS, false, 1, {RT_T, RT_NONE}, {}, {}};
            e.fwd = {{RT_T, NT, false, 0, 0, 0, false, false}, {RT_S, NS, true, 0, 0, 0, false, false}};
            e.bwd = {{RT_T, NT, false, 0, 0, 0, false, false}, {RT_S, NS, true, 0, 0, 0, false, true}};
            break;
        case LT2L:      // key = LN1(cat[sos, targets]); key rows [0, NS) come from the same LN as the query
            e = {NS, NS + NT, false, 1, {RT_S, RT_NONE}, {}, {}};
            e.fwd = {{RT_S, NS, false, 0, 0, 0, false, false}, {RT_S, NS, true, NS, NS + NT, 0, false, false}, {RT_T, NT, true, NT, NS + NT, NS, false, false}};
            e.bwd = {{RT_S, NS, true, NS, NS + NT, 0, true, false}, {RT_T, NT, true, NT, NS + NT, NS, false, true}};
            break;
        default:        // maskgit: query = key = LN1(cat[contexts, targets]); the output is split back into both streams
            e = {NC + NT, NC + NT, true, 2, {RT_C, RT_T}, {}, {}};
            e.fwd = {{RT_C, NC, false, NC, NC + NT, 0, false, false}, {RT_T, NT, false, NT, NC + NT, NC, false, false}};
            e.bwd = e.fwd;
            break;
    }
    return e;
}

void compare_jobs(const char* what, const std::vector<Job>& want, const RouteSeg* got, int n, int mode, int NS, int NC, int NT) {
    if ((int)want.size() != n) { fail(what, mode, NS, NC, NT, (long)want.size(), n); return; }
    for (int j = 0; j < n; ++j) {
        const Job& w = want[j];
        const RouteSeg& g = got[j];
        if (w.stream != g.stream || w.len != g.len || w.key != g.key || w.seg != g.seg || w.stride != g.stride || w.off != g.off ||
            w.add_q != g.add_q || w.key_only != g.key_only)
            fail(what, mode, NS, NC, NT, j, g.stream);
    }
}

void check_block(int mode, int NS, int NC, int NT) {
    const Expect e = by_hand(mode, NS, NC, NT);
    const Route& r = route_of(mode);
    const int len[RT_STREAMS] = {NS, NC, NT};
    if (route_rows(r.q, len) != e.NQ) fail("NQ", mode, NS, NC, NT, e.NQ, route_rows(r.q, len));
    if (route_rows(r.k, len) != e.NK) fail("NK", mode, NS, NC, NT, e.NK, route_rows(r.k, len));
    if (r.self != e.fused) fail("fused QKV", mode, NS, NC, NT);
    if (r.nq() != e.nout || r.q[0] != e.out[0] || r.q[1] != e.out[1]) fail("output streams", mode, NS, NC, NT, r.q[0], r.q[1]);
    RouteSeg got[RT_MAXJ + 1];
    compare_jobs("forward LN1 jobs", e.fwd, got, route_fwd_segs(r, len, got), mode, NS, NC, NT);
    compare_jobs("backward LN1 jobs", e.bwd, got, route_bwd_jobs(r, len, got), mode, NS, NC, NT);
}

// liveness as the per-mode switch had it: gS / gT = "the gradient of the latents / targets stream is defined above this block"
void check_liveness(const int32_t* modes, int n) {
    char want[MEBT_MAX_LAYERS] = {0}, got[MEBT_MAX_LAYERS] = {0};
    bool tok = false, mgit = false, gS = false, gT = true;
    for (int i = n - 1; i >= 0; --i) {
        switch (modes[i]) {
            case ENC: if (gS) { want[i] = 1; tok = true; } break;
            case SELF: if (gS) want[i] = 1; break;
            case LT2L: if (gS) { want[i] = 1; gT = true; } break;
            case DEC: if (gT) { want[i] = 1; gS = true; } break;
            case MG: want[i] = 1; tok = true; mgit = true; break;
        }
    }
    bool tok_live = false, two_q = false;
    route_liveness(modes, n, got, tok_live, two_q);
    for (int i = 0; i < n; ++i)
        if (want[i] != got[i]) fail("live", -1, n, i, modes[i], want[i], got[i]);
    if (tok != tok_live) fail("tok_live", -1, n, 0, 0, tok, tok_live);
    if (mgit != two_q) fail("has_maskgit", -1, n, 0, 0, mgit, two_q);
}

}  // namespace

int main() {
    int cases = 0;
    const int NSs[] = {0, 8, 256}, NCs[] = {0, 5, 7936}, NTs[] = {1, 7, 256};
    for (int mode = 0; mode < 5; ++mode)
        for (int NS : NSs) {
            if (NS == 0 && mode != MG) continue;      // sos_emb = 0 is accepted for all-maskgit models only
            for (int NC : NCs)
                for (int NT : NTs) {
                    check_block(mode, NS, NC, NT);
                    ++cases;
                }
        }
    for (int n = 1; n <= 6; ++n) {
        int count = 1;
        for (int i = 0; i < n; ++i) count *= 5;
        for (int c = 0; c < count; ++c, ++cases) {
            int32_t modes[6];
            for (int i = 0, v = c; i < n; ++i, v /= 5) modes[i] = v % 5;
            check_liveness(modes, n);
        }
    }
    {   // the shipped 24-block list: every block is live, the token embedding gets a gradient, no block rewrites two streams
        const int32_t sky[24] = {ENC, SELF, ENC, SELF, ENC, SELF, ENC, SELF, ENC, SELF, ENC, SELF, ENC,
                                 DEC, LT2L, DEC, LT2L, DEC, LT2L, DEC, LT2L, DEC, LT2L, DEC};
        char live[24];
        bool tok_live = false, two_q = true;
        route_liveness(sky, 24, live, tok_live, two_q);
        for (int i = 0; i < 24; ++i)
            if (live[i] != 1) fail("shipped list: dead block", -1, 24, i, sky[i]);
        if (!tok_live || two_q) fail("shipped list: tok_live / has_maskgit", -1, 24, 0, 0, tok_live, two_q);
        check_liveness(sky, 24);
        ++cases;
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok: %d cases\n", cases);
    return 0;
}
