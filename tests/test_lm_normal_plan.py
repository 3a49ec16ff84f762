"""The launch plan of the LM normal equations as kernels/syrk.hip computes it.  The plan is not
restated here: tests/cpp/lm_normal_plan_table.cpp includes csrc/lm_normal_plan.hpp -- the header
syrk.hip takes its tile counts, K split, workspace sizes and LevMarqMPI's exchange layout from --
and prints it for every rank, which these tests read.  They check it against the definitions
(written here: what the kernels index, what a partition is), and the K split and the allgather
slot against the values of the commit before the header existed (tests/golden/lm_normal_plan_parent.json,
printed once by a throw-away program holding that commit's slice_cfg arithmetic)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NS = (65, 128, 129, 257, 300, 2048)
MS = (64, 65, 777, 4100, 16384)
PS = tuple(range(1, 9))
SUBS = (0, 1, 2, 3, 4, 64)   # 0: PNOL_SYRK_SUB unset
PCTS = (0, 50, 75, 100)
TILE, TK, SLICES, MAXNODES = 128, 16, 8, 4
E = TILE * TILE

RANK_FIELDS = ("r ok nt ntiles ntiles64 mS sub kfirst kchunk split per_tile s0 s1 tpr slot t0 cnt part_all "
               "part_tiles part_slices jtr nodes recv packed slot_off jtf_off nn").split()


class Plan:
    def __init__(self, key):
        self.key = key
        self.const, self.ranks, self.nodes, self.first = None, [], [], None
        self.merge, self.jtf, self.x = {}, {}, {}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lm_plan") / "lm_normal_plan_table")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I",
                    os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "lm_normal_plan_table.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    out, p = {}, None
    for line in r.stdout.decode().splitlines():
        tag, _, rest = line.partition(" ")
        v = [int(x) for x in rest.split()]
        if tag == "x":
            p.x.setdefault((v[0], v[1], v[2]), []).append((v[3], v[4], v[5]))
        elif tag == "merge":
            p.merge[(v[0], v[1])] = (v[2], v[3])
        elif tag == "jtf":
            p.jtf[(v[0], v[1])] = v[2]
        elif tag == "rank":
            p.ranks.append(dict(zip(RANK_FIELDS, v)))
        elif tag == "node":
            assert v[0] == len(p.nodes)
            p.nodes.append((v[1], v[2], v[3]))
        elif tag == "first":
            p.first = v
        elif tag == "const":
            p.const = tuple(v)
        else:
            assert tag == "plan", line
            p = out[tuple(v)] = Plan(tuple(v))
    assert set(out) == {(n, m, P, f, pct) for n in NS for m in MS for P in PS for f in SUBS for pct in PCTS}
    return out


def ceil_div(a, b):
    return -(-a // b)


def test_tiles_slices_and_chunks(plans):
    for (n, m, P, f, pct), p in plans.items():
        assert p.const == (TILE, TK, SLICES, MAXNODES)
        assert [r["r"] for r in p.ranks] == list(range(P))
        nt, nt64 = ceil_div(n, TILE), ceil_div(n, 64)
        for r in p.ranks:
            assert r["ok"] == 1
            assert (r["nt"], r["ntiles"], r["ntiles64"]) == (nt, nt * (nt + 1) // 2, nt64 * (nt64 + 1) // 2)
            assert r["mS"] % 64 == 0 and SLICES * r["mS"] >= m, (p.key, r)
            assert r["sub"] >= 1 and r["kfirst"] % TK == 0 and r["kchunk"] % TK == 0, (p.key, r)
            assert r["kfirst"] > 0 and r["kchunk"] > 0
            assert r["kfirst"] + (r["sub"] - 1) * r["kchunk"] >= r["mS"], (p.key, r)   # the chunks cover a slice
            assert r["split"] == SLICES * r["sub"] and r["per_tile"] == r["split"] * E
            # the K split never depends on the rank or on P (every element summed the same way)
            q = plans[(n, m, 1, f, pct)].ranks[0]
            assert all(r[k] == q[k] for k in ("mS", "sub", "kfirst", "kchunk"))


def test_rank_slices_and_dyadic_nodes(plans):
    for (n, m, P, f, pct), p in plans.items():
        # the ranks' slice ranges partition 0 .. 7, in rank order
        assert p.ranks[0]["s0"] == 0 and p.ranks[-1]["s1"] == SLICES
        assert all(a["s1"] == b["s0"] for a, b in zip(p.ranks, p.ranks[1:]))
        assert all(r["s0"] < r["s1"] for r in p.ranks)
        assert p.first[0] == 0 and p.first[P] == len(p.nodes) and len(p.first) == P + 1
        for r in p.ranks:
            mine = p.nodes[p.first[r["r"]]:p.first[r["r"] + 1]]
            assert r["nn"] == len(mine) and 1 <= len(mine) <= MAXNODES, (p.key, r)
            assert all(o == r["r"] for _, _, o in mine)
            # inside the rank's range, aligned to their width, in slice order without gaps
            pos = r["s0"]
            for lo, w, _ in mine:
                assert lo == pos and w in (1, 2, 4, 8) and lo % w == 0 and lo + w <= r["s1"], (p.key, mine)
                pos = lo + w
            assert pos == r["s1"]
            # they are the nodes k_tree_nodes writes: the range's leaves merged by the sibling rule
            sz = [1 if r["s0"] <= i < r["s1"] else 0 for i in range(SLICES)]
            sibling_merge(sz)
            assert [(i, sz[i]) for i in range(SLICES) if sz[i]] == [(lo, w) for lo, w, _ in mine]
        # the nodes of all ranks merge to the single root
        sz = [0] * SLICES
        for lo, w, _ in p.nodes:
            assert sz[lo] == 0
            sz[lo] = w
        sibling_merge(sz)
        assert sz == [SLICES] + [0] * (SLICES - 1), (p.key, p.nodes)


def sibling_merge(sz):
    """tree_merge of syrk.hip on the widths: siblings of equal width merge, bottom up."""
    w = 1
    while w < SLICES:
        for i in range(0, SLICES, 2 * w):
            if sz[i] == w and sz[i + w] == w:
                sz[i], sz[i + w] = 2 * w, 0
        w *= 2


def test_tile_owners_and_allgather_slots(plans):
    for (n, m, P, f, pct), p in plans.items():
        ntiles = p.ranks[0]["ntiles"]
        tpr = ceil_div(ntiles, P)
        owned = []
        for r in p.ranks:
            assert r["tpr"] == tpr and 0 <= r["cnt"] <= tpr
            owned += list(range(r["t0"], r["t0"] + r["cnt"]))
            # a slot: the rank's tpr tiles, then kMaxNodes -J^T F nodes of n doubles; P slots
            assert r["slot"] == tpr * E + MAXNODES * n and r["packed"] == P * r["slot"]
            assert r["slot_off"] == r["r"] * r["slot"] and r["jtf_off"] == tpr * E
        assert owned == list(range(ntiles)), p.key   # the owners' ranges partition the tiles
        # k_syrk_unpack reads tile t at (t / tpr) * slot + (t % tpr) * 128^2: where its owner's merge wrote it
        slot = p.ranks[0]["slot"]
        for r in p.ranks:
            for t in range(r["t0"], r["t0"] + r["cnt"]):
                assert (t // tpr) * slot + (t % tpr) * E == r["slot_off"] + (t - r["t0"]) * E, (p.key, t)
        # the -J^T F table reads node c where its rank's k_tree_nodes wrote it (node i of rank q at
        # q's slot + tpr * 128^2 + i * n), the same on every rank
        for r in p.ranks:
            for c, (lo, w, q) in enumerate(p.nodes):
                i = c - p.first[q]
                assert 0 <= i < MAXNODES
                assert p.jtf[(r["r"], c)] == q * slot + tpr * E + i * n, (p.key, r["r"], c)


def test_exchange_blocks(plans):
    for (n, m, P, f, pct), p in plans.items():
        ntiles, tpr = p.ranks[0]["ntiles"], p.ranks[0]["tpr"]
        for d in p.ranks:
            got = []   # (roff, count) of everything owner d receives
            for q in p.ranks:
                if q["r"] == d["r"]:
                    continue
                sent = p.x.get((q["r"], q["r"], d["r"]), [])
                assert sent == p.x.get((d["r"], q["r"], d["r"]), []), p.key   # both ends list the same blocks
                assert len(sent) == (q["nn"] if d["cnt"] else 0)
                for i, (soff, roff, count) in enumerate(sent):
                    c = p.first[q["r"]] + i
                    assert count == d["cnt"] * E
                    # q's node i of tile t sits at (i * ntiles + t) * 128^2 of "lm_nodes" (k_tree_nodes)
                    assert soff == (i * ntiles + d["t0"]) * E and soff + count <= q["nodes"], (p.key, q, d)
                    assert roff == c * tpr * E and roff + count <= d["recv"], (p.key, q, d)
                    got.append((roff, count))
                    # the owner's merge reads it there
                    assert p.merge[(d["r"], c)] == (0, roff)
            got.sort()
            assert all(a[0] + a[1] <= b[0] for a, b in zip(got, got[1:])), (p.key, d["r"], got)
            # and its own nodes in place
            for c in range(p.first[d["r"]], p.first[d["r"] + 1]):
                off = ((c - p.first[d["r"]]) * ntiles + d["t0"]) * E
                assert p.merge[(d["r"], c)] == (1, off) and off + d["cnt"] * E <= d["nodes"]


def test_workspace_counts(plans):
    for (n, m, P, f, pct), p in plans.items():
        for r in p.ranks:
            ntiles, sub, nt = r["ntiles"], r["sub"], r["nt"]
            # syrk_partials writes part[((t - tile0) * nsl * sub + (s - slice0) * sub + u) * 128^2 + e]:
            # the largest index + 1 is ntl * nsl * sub * 128^2
            assert r["part_all"] == ntiles * SLICES * sub * E                 # the whole matrix
            for rb in range(nt):                                               # launch_jtj_rows: rows [rb, re)
                for re_ in range(rb + 1, nt + 1):
                    t0, t1 = rb * (rb + 1) // 2, re_ * (re_ + 1) // 2
                    end = t0 * r["per_tile"] + (t1 - t0) * SLICES * sub * E
                    assert end <= r["part_all"] and (re_ < nt or end == r["part_all"])
            if r["cnt"]:                                                       # launch_jtj_sharded: its tiles
                assert r["part_tiles"] == r["cnt"] * SLICES * sub * E
            else:
                assert r["part_tiles"] > 0
            assert r["part_slices"] == ntiles * (r["s1"] - r["s0"]) * sub * E  # lm_normal_core: its slices
            assert r["jtr"] == SLICES * n
            assert r["nodes"] == r["nn"] * ntiles * E and r["recv"] == len(p.nodes) * r["tpr"] * E


def test_matches_parent_commit(plans):
    """The header against the launchers it replaced: (mS, sub, kfirst, kchunk) and (tpr, slot) as the
    parent commit's inline arithmetic gave them."""
    with open(os.path.join(ROOT, "tests", "golden", "lm_normal_plan_parent.json")) as fh:
        gold = json.load(fh)
    cfg = {tuple(row[:4]): tuple(row[4:]) for row in gold["slice_cfg"]}
    own = {tuple(row[:2]): tuple(row[2:]) for row in gold["owner"]}
    assert set(cfg) == {(n, m, f, pct) for n in NS for m in MS for f in SUBS for pct in PCTS}
    assert set(own) == {(n, P) for n in NS for P in PS}
    for (n, m, P, f, pct), p in plans.items():
        for r in p.ranks:
            assert (r["mS"], r["sub"], r["kfirst"], r["kchunk"]) == cfg[(n, m, f, pct)], p.key
            assert (r["tpr"], r["slot"]) == own[(n, P)], p.key
