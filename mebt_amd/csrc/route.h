// How the five block modes route the three token streams (reference gpt.py:170-192), as one table, and everything the engine derives
// from it: attention shape, the LN1 segments of forward and backward, which streams a block rewrites, which blocks the loss reaches.
// Host only, no HIP types: engine.cpp sequences launches from these lists; tests/engine_route_walk.cpp compares them with the
// per-mode cases written out by hand.
#pragma once
#include <initializer_list>

#include "../../include/mebt_hip.h"

enum { RT_S = 0, RT_C = 1, RT_T = 2, RT_STREAMS = 3, RT_NONE = -1 };      // latents (sos), contexts, targets
constexpr int RT_MAXJ = 3;      // LN1 jobs of one block, forward or backward (one launch: MEBT_LN_MAXJ of kernels.h)

struct Route {
    int q[2], k[2];     // the streams whose rows, concatenated, are the query / the key rows (RT_NONE: unused)
    bool self;          // the key is the query: one LN1, one fused QKV product
    constexpr int nq() const { return (q[0] != RT_NONE) + (q[1] != RT_NONE); }
    constexpr int nk() const { return (k[0] != RT_NONE) + (k[1] != RT_NONE); }
    constexpr bool q_has(int s) const { return q[0] == s || q[1] == s; }
    constexpr int segments() const { return nq() + (self ? 0 : nk()); }
};

constexpr Route ROUTES[5] = {
    {{RT_S, RT_NONE}, {RT_C, RT_NONE}, false},     // latent_enc:  latents read the contexts
    {{RT_S, RT_NONE}, {RT_S, RT_NONE}, true},      // latent_self
    {{RT_T, RT_NONE}, {RT_S, RT_NONE}, false},     // latent_dec:  targets read the latents
    {{RT_S, RT_NONE}, {RT_S, RT_T}, false},        // lt2l:        latents read cat[latents, targets]
    {{RT_C, RT_T}, {RT_C, RT_T}, true},            // maskgit:     full attention over cat[contexts, targets]
};
static_assert(MEBT_MODE_LATENT_ENC == 0 && MEBT_MODE_LATENT_SELF == 1 && MEBT_MODE_LATENT_DEC == 2 && MEBT_MODE_LT2L == 3 &&
                  MEBT_MODE_MASKGIT == 4, "ROUTES is indexed by mebt_mode");
static_assert(ROUTES[0].segments() <= RT_MAXJ && ROUTES[1].segments() <= RT_MAXJ && ROUTES[2].segments() <= RT_MAXJ &&
                  ROUTES[3].segments() <= RT_MAXJ && ROUTES[4].segments() <= RT_MAXJ, "a block's LN1 jobs must fit one launch");
inline const Route& route_of(int mode) { return ROUTES[mode]; }

// rows per sample of a side (len: the three stream lengths NS, NC, NT)
inline int route_rows(const int ids[2], const int len[RT_STREAMS]) {
    return (ids[0] != RT_NONE ? len[ids[0]] : 0) + (ids[1] != RT_NONE ? len[ids[1]] : 0);
}

// One LN1 job: `len` rows per sample of `stream`, which are rows [off, off + len) of every `stride` rows of the side's buffer
// (seg = stride = off = 0: the stream is the whole side).
struct RouteSeg {
    int stream, len;
    bool key;                   // forward: the key side's buffers; backward: dy and the statistics of the key side
    int seg, stride, off;
    bool add_q = false;         // backward: the stream is also the whole query, dy2 = the query side's gradient
    bool key_only = false;      // backward: accumulates when the stream's gradient is already defined, skipped when it has no rows
};

inline int route_side_segs(const int ids[2], const int len[RT_STREAMS], bool key, RouteSeg* out) {
    const bool two = ids[1] != RT_NONE;
    const int total = route_rows(ids, len);
    int n = 0, off = 0;
    for (int j = 0; j < 2 && ids[j] != RT_NONE; ++j) {
        out[n++] = {ids[j], len[ids[j]], key, two ? len[ids[j]] : 0, two ? total : 0, two ? off : 0};
        off += len[ids[j]];
    }
    return n;
}

// forward: the query streams, then the key streams unless the key is the query
inline int route_fwd_segs(const Route& r, const int len[RT_STREAMS], RouteSeg out[RT_MAXJ]) {
    int n = route_side_segs(r.q, len, false, out);
    if (!r.self) n += route_side_segs(r.k, len, true, out + n);
    return n;
}

// backward: one job per query stream, then one per stream that only the key reads.  A query stream that is also a key segment of a
// non-self block (lt2l's latents) went through ONE LayerNorm that fed both sides: its job is the key segment with the query
// gradient added.
inline int route_bwd_jobs(const Route& r, const int len[RT_STREAMS], RouteSeg out[RT_MAXJ]) {
    RouteSeg q[2], k[2];
    const int nq = route_side_segs(r.q, len, false, q), nk = r.self ? 0 : route_side_segs(r.k, len, true, k);
    int n = 0;
    for (int j = 0; j < nq; ++j) {
        out[n] = q[j];
        for (int i = 0; i < nk; ++i)
            if (k[i].stream == q[j].stream) { out[n] = k[i]; out[n].add_q = true; }
        ++n;
    }
    for (int i = 0; i < nk; ++i)
        if (!r.q_has(k[i].stream) && k[i].len > 0) { out[n] = k[i]; out[n++].key_only = true; }
    return n;
}

// Which blocks the loss reaches: the head reads the targets only, so walk down from the top with defined = {T}; a block whose query
// has a defined stream is live and defines every stream it reads.  tok_live: the contexts' gradient (the token embedding's only
// one) gets defined; two_q: some block rewrites two streams.
inline void route_liveness(const int32_t* modes, int n, char* live, bool& tok_live, bool& two_q) {
    bool def[RT_STREAMS] = {false, false, true};
    tok_live = two_q = false;
    for (int i = n - 1; i >= 0; --i) {
        const Route& r = route_of(modes[i]);
        if (r.nq() == 2) two_q = true;
        live[i] = (def[r.q[0]] || (r.q[1] != RT_NONE && def[r.q[1]])) ? 1 : 0;
        if (!live[i]) continue;
        for (int s : {r.q[0], r.q[1], r.k[0], r.k[1]})
            if (s != RT_NONE) def[s] = true;
        if (def[RT_C]) tok_live = true;
    }
}
