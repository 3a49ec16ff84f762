// lm_normal_plan.hpp -- the launch plan of the LM normal equations (kernels/syrk.hip), in plain
// host C++17 with no HIP include: every count, size and offset the J^T J launchers and
// LevMarqMPI's tile exchange use, from (m, n, P, rank) alone.  syrk.hip includes it, and
// tests/cpp/lm_normal_plan_table.cpp prints it for tests/test_lm_normal_plan.py.  The environment
// is not read here: syrk.hip reads PNOL_SYRK_SUB / PNOL_SYRK_FIRST and passes the values in.
#pragma once

#include <algorithm>
#include <cstddef>

namespace pnol {

constexpr int kLmSlices = 8;   // the LM m-slices (pnol_internal.hpp), of lm_slice_rows(m) rows each
inline int lm_slice_rows(int m) { return (((m + kLmSlices - 1) / kLmSlices) + 63) / 64 * 64; }
// rank r of P (<= kLmSlices) holds slices [floor(r 8 / P), floor((r + 1) 8 / P))
inline void lm_rank_slices(int P, int r, int* s0, int* s1) { *s0 = r * kLmSlices / P, *s1 = (r + 1) * kLmSlices / P; }

constexpr int kTile = 128;   // J^T J output tile (rows = columns)
constexpr int kTK = 16;      // K columns per LDS stage
// dyadic nodes of one rank's slice range, at most ([1, 7) of the 8-leaf tree: 1, 2-3, 4-5, 6);
// every rank's allgather slot keeps room for this many -J^T F nodes (checked by lm_normal_plan)
constexpr int kMaxNodes = 4;

// K split: kLmSlices m-slices of mS rows (a multiple of 64, so an FD row panel never straddles
// two), each cut into `sub` chunks: chunk 0 of kfirst columns, the others of kchunk.
struct SliceCfg { int mS, sub, kfirst, kchunk; };
// a block of doubles of a point-to-point exchange: soff in the sender's buffer, roff in the receiver's
struct XBlock { size_t soff, roff, count; };

struct LmNormalPlan {
    static constexpr long E = (long)kTile * kTile;   // doubles per tile
    int m = 0, n = 0, P = 1, rank = 0;
    int nt = 0, ntiles = 0, ntiles64 = 0;   // 128-row tile rows, lower-triangle tiles, 64 x 64 ones (T64)
    SliceCfg sc{};
    int split = 0;       // K split of a whole-matrix launch: kLmSlices * sub
    long per_tile = 0;   // doubles of one tile's whole-matrix partials: split * E
    int s0 = 0, s1 = kLmSlices;   // this rank's m-slices (lm_rank_slices)
    // The global node list: rank q's dyadic nodes (first slice, width) of the slice tree inside its
    // range, in slice order, ranks in order; rank q's are [first[q], first[q + 1]).
    int NC = 0, node_lo[kLmSlices] = {}, node_w[kLmSlices] = {}, owner[kLmSlices] = {}, first[kLmSlices + 1] = {};
    // Tile owners: contiguous ranges of tpr = ceil(ntiles / P) tiles.  An allgather slot holds a
    // rank's tpr summed tiles, then its (up to kMaxNodes) -J^T F nodes of n doubles each.
    int tpr = 0;
    long slot = 0;
    bool ok = false;   // the m-slice plan holds: P <= kLmSlices and no rank has more than kMaxNodes nodes

    int nsl() const { return s1 - s0; }
    int nn() const { return first[rank + 1] - first[rank]; }   // this rank's nodes
    int t0_of(int d) const { return std::min(ntiles, d * tpr); }
    int cnt_of(int d) const { return std::min(ntiles, t0_of(d) + tpr) - t0_of(d); }
    // Element counts of the workspace buffers: "syrk_part" for ntl tiles x nsl_ m-slices (an empty
    // range still gets one; default the whole matrix), "jtr_part", "lm_nodes", "lm_nodes_recv", "lm_packed"
    size_t part_elems(int ntl, int nsl_) const { return (size_t)std::max(ntl, 1) * std::max(nsl_, 1) * sc.sub * E; }
    size_t part_elems() const { return part_elems(ntiles, kLmSlices); }
    size_t jtr_elems() const { return (size_t)kLmSlices * n; }
    size_t nodes_elems() const { return (size_t)std::max(nn(), 1) * ntiles * E; }
    size_t recv_elems() const { return (size_t)NC * tpr * E; }
    size_t packed_elems() const { return (size_t)P * slot; }
    // "lm_nodes": its rank's node c (global index) of tile t; "lm_nodes_recv": node c of the
    // owner's tiles; "lm_packed": rank d's slot, its -J^T F nodes behind its tiles.
    long node_off(int c, int t) const { return ((long)(c - first[owner[c]]) * ntiles + t) * E; }
    long recv_off(int c) const { return (long)c * tpr * E; }
    long slot_off(int d) const { return (long)d * slot; }
    long jtf_off() const { return (long)tpr * E; }   // inside a slot
    long jtf_node_off(int c) const { return slot_off(owner[c]) + jtf_off() + (long)(c - first[owner[c]]) * n; }
    // where the owner's merge reads node c of its tiles: its own nodes in place ("lm_nodes"), the
    // others' where the exchange put them ("lm_nodes_recv")
    bool merge_local(int c) const { return owner[c] == rank; }
    long merge_off(int c) const { return merge_local(c) ? node_off(c, t0_of(rank)) : recv_off(c); }
    // The tree-order exchange (a reduce-scatter): what rank q sends to owner d -- each of q's
    // nodes of d's tiles, from q's "lm_nodes" into d's "lm_nodes_recv"; each block goes to put(XBlock).
    template <typename Put>
    void exchange_blocks(int q, int d, Put put) const {
        for (int c = first[q]; c < first[q + 1] && cnt_of(d) > 0; ++c)
            put(XBlock{(size_t)node_off(c, t0_of(d)), (size_t)recv_off(c), (size_t)cnt_of(d) * E});
    }
};

// forced_sub: PNOL_SYRK_SUB (0: unset); first_pct: PNOL_SYRK_FIRST (75 when unset)
inline LmNormalPlan lm_normal_plan(int m, int n, int P, int rank, int forced_sub, int first_pct) {
    LmNormalPlan p;
    p.m = m, p.n = n, p.P = P, p.rank = rank;
    p.nt = (n + kTile - 1) / kTile;
    p.ntiles = p.nt * (p.nt + 1) / 2;
    p.ntiles64 = ((n + 63) / 64) * ((n + 63) / 64 + 1) / 2;
    // sub depends on (m, n) only -- never on the number of ranks -- so every A element is summed
    // the same way on any P.  Default: enough workgroups to fill the chip (>= 2048 = 256 CUs x 2
    // resident x 4 rounds), chunks >= 256 columns.  At m = 16384, n = 2048 (136 tiles) sub = 2:
    // 2176 workgroups of K = 1024 (measured: SYRK 1.33 ms + reduce 0.09 ms, vs 1.42 + 0.05 ms at
    // sub = 1).  forced_sub > 0 overrides.
    SliceCfg& c = p.sc;
    c.mS = lm_slice_rows(m);
    const int want = (2048 + p.ntiles * kLmSlices - 1) / (p.ntiles * kLmSlices), cap = std::max(1, c.mS / 256);
    c.sub = forced_sub > 0 ? std::min(forced_sub, std::max(1, c.mS / kTK)) : std::max(1, std::min(want, cap));
    c.kfirst = c.kchunk = ((c.mS + c.sub - 1) / c.sub + kTK - 1) / kTK * kTK;
    // Chunk 0 takes 75% of the slice (first_pct; the rest split evenly over chunks 1..sub-1) and
    // is dispatched first (k_syrk_tile's order): 1088 long workgroups, then 1088 short ones that
    // fill the tail of the last dispatch round.  Measured at m = 16384, n = 2048: 1.265 ms vs
    // 1.326 ms for two equal chunks (tools/syrk_sweep.py).
    if (c.sub >= 2 && first_pct > 0 && first_pct < 100) {
        c.kfirst = std::max(kTK, (int)((long)c.mS * first_pct / 100) / kTK * kTK);
        c.kchunk = ((c.mS - c.kfirst + c.sub - 2) / (c.sub - 1) + kTK - 1) / kTK * kTK;
    }
    p.split = kLmSlices * c.sub;
    p.per_tile = (long)p.split * LmNormalPlan::E;
    if (P < 1 || rank < 0 || rank >= P) return p;
    p.tpr = (p.ntiles + P - 1) / P;
    p.slot = (long)p.tpr * LmNormalPlan::E + (long)kMaxNodes * n;
    if (P > kLmSlices) return p;   // tile owners only (launch_jtj_sharded): no m-slice per rank
    lm_rank_slices(P, rank, &p.s0, &p.s1);
    p.ok = true;
    for (int q = 0, a, b; q < P; ++q) {
        lm_rank_slices(P, q, &a, &b);
        for (int i = a, w; i < b; i += w, ++p.NC) {   // the widest aligned node that starts at slice i
            for (w = 1; i % (2 * w) == 0 && i + 2 * w <= b && 2 * w <= kLmSlices;) w *= 2;
            p.node_lo[p.NC] = i, p.node_w[p.NC] = w, p.owner[p.NC] = q;
        }
        if (p.NC - p.first[q] > kMaxNodes) p.ok = false;
        p.first[q + 1] = p.NC;
    }
    return p;
}

}  // namespace pnol
