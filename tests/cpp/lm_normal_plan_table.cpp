// Prints the LM normal equations' launch plan as kernels/syrk.hip computes it
// (csrc/lm_normal_plan.hpp, the header syrk.hip includes) for tests/test_lm_normal_plan.py.
//   lm_normal_plan_table n m P forced_sub first_pct     that one plan (every rank)
//   lm_normal_plan_table                                the sweep: n in {65, 128, 129, 257, 300, 2048},
//       m in {64, 65, 777, 4100, 16384}, P = 1 .. 8, forced_sub in {0 (unset), 1, 2, 3, 4, 64},
//       first_pct in {0, 50, 75, 100}
// Output, one record per line (counts and offsets in doubles):
//   plan <n> <m> <P> <forced_sub> <first_pct>
//   const <kTile> <kTK> <kLmSlices> <kMaxNodes>
//   rank <r> <ok> <nt> <ntiles> <ntiles64> <mS> <sub> <kfirst> <kchunk> <split> <per_tile> <s0> <s1> <tpr>
//        <slot> <t0> <cnt> <part whole> <part of its tile range> <part of its slices> <jtr> <lm_nodes>
//        <lm_nodes_recv> <lm_packed> <slot_off> <jtf_off> <nn>
//   node <c> <first slice> <width> <owner>            the global node list (rank 0's plan)
//   first <first[0]> .. <first[P]>
//   merge <r> <c> <local> <off>      where owner r's merge reads node c ("lm_nodes" if local, else "lm_nodes_recv")
//   jtf <r> <c> <off>                where rank r's -J^T F table reads node c in "lm_packed"
//   x <r> <q> <d> <soff> <roff> <count>   rank r's plan: a block rank q sends to owner d (q or d = r)
#include <cstdio>
#include <cstdlib>

#include "lm_normal_plan.hpp"

static void plan(int n, int m, int P, int forced, int pct) {
    using namespace pnol;
    std::printf("plan %d %d %d %d %d\nconst %d %d %d %d\n", n, m, P, forced, pct, kTile, kTK, kLmSlices, kMaxNodes);
    for (int r = 0; r < P; ++r) {
        const LmNormalPlan p = lm_normal_plan(m, n, P, r, forced, pct);
        std::printf("rank %d %d %d %d %d %d %d %d %d %d %ld %d %d %d %ld %d %d %zu %zu %zu %zu %zu %zu %zu %ld %ld %d\n", r,
                    (int)p.ok, p.nt, p.ntiles, p.ntiles64, p.sc.mS, p.sc.sub, p.sc.kfirst, p.sc.kchunk, p.split,
                    p.per_tile, p.s0, p.s1, p.tpr, p.slot, p.t0_of(r), p.cnt_of(r), p.part_elems(),
                    p.part_elems(p.cnt_of(r), kLmSlices), p.part_elems(p.ntiles, p.nsl()), p.jtr_elems(),
                    p.nodes_elems(), p.recv_elems(), p.packed_elems(), p.slot_off(r), p.jtf_off(), p.nn());
        if (r == 0) {
            for (int c = 0; c < p.NC; ++c) std::printf("node %d %d %d %d\n", c, p.node_lo[c], p.node_w[c], p.owner[c]);
            std::printf("first");
            for (int q = 0; q <= P; ++q) std::printf(" %d", p.first[q]);
            std::printf("\n");
        }
        for (int c = 0; c < p.NC; ++c) {
            std::printf("merge %d %d %d %ld\n", r, c, (int)p.merge_local(c), p.merge_off(c));
            std::printf("jtf %d %d %ld\n", r, c, p.jtf_node_off(c));
        }
        for (int q = 0; q < P; ++q)
            for (int d = 0; d < P; ++d) {
                if (q == d || (q != r && d != r)) continue;   // what rank r itself sends and receives
                p.exchange_blocks(q, d, [&](const XBlock& b) {
                    std::printf("x %d %d %d %zu %zu %zu\n", r, q, d, b.soff, b.roff, b.count);
                });
            }
    }
}

int main(int argc, char** argv) {
    if (argc == 6) {
        plan(std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
        return 0;
    }
    const int ns[] = {65, 128, 129, 257, 300, 2048}, ms[] = {64, 65, 777, 4100, 16384};
    const int subs[] = {0, 1, 2, 3, 4, 64}, pcts[] = {0, 50, 75, 100};
    for (int n : ns)
        for (int m : ms)
            for (int P = 1; P <= 8; ++P)
                for (int f : subs)
                    for (int pct : pcts) plan(n, m, P, f, pct);
    return 0;
}
