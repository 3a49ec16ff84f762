"""The persistent Cholesky's worker claim order as the kernel computes it, and a claim-queue
simulation of the persistent launch.  The order is not restated here: tests/cpp/chol_claim_table.cpp
includes csrc/chol_tasks.hpp -- the header kernels/chol.hip takes task_of, the task counts and
the worker guard from -- and prints the claim table g -> (k, i, j, h), which these tests read.
The simulation models the waits of k_chol_persist: workers claim task indices in order, each
waits until its dependencies are published (the kernel's spin waits), and the diagonal chain
steps when its two tiles are ready.  Checks that the claim order is a permutation of the step
tasks (written here from their definition) and that every order the library uses drains -- step
order with any worker count, order 1 from the worker count at which the guard
(chol_claim_order) keeps it; below that the kernel falls back to step order."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ClaimTables:
    """One run of chol_claim_table: tables[(T, order, split, rowmajor)] = [(k, i, j, h), ...] by
    claim index, need[split] = the smallest worker count at which the guard keeps order 1,
    guard[split][w] = the order used with w workers when order 1 is requested."""

    def __init__(self, text):
        self.tables, self.need, self.guard = {}, {}, {}
        lines = iter(text.splitlines())
        for line in lines:
            f = line.split()
            if f[0] == "guard":
                split = bool(int(f[1]))
                self.need[split] = int(f[2])
                self.guard[split] = [int(x) for x in f[3:]]
            else:
                assert f[0] == "table", line
                T, order, split, rowmajor, nt = (int(x) for x in f[1:])
                self.tables[(T, order, bool(split), bool(rowmajor))] = [
                    tuple(int(x) for x in next(lines).split()) for _ in range(nt)]


@pytest.fixture(scope="module")
def claims(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chol_claim") / "chol_claim_table")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I",
                    os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "chol_claim_table.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe, "2", "35"], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    return ClaimTables(r.stdout.decode())


def all_tasks(T, split):
    """The step tasks by definition: step k's panel rows i = k+1 .. T-1 and its update tiles (i, j),
    k+1 <= j <= i <= T-1, except the chain's own (k+1, k+1); with the split critical updates (and at
    least two panel rows) the tiles (k+2, k+1) and (k+2, k+2) as halves 0 and 1."""
    out = []
    for k in range(T - 1):
        out += [(k, i, -1, -1) for i in range(k + 1, T)]
        for i in range(k + 1, T):
            for j in range(k + 1, i + 1):
                if (i, j) == (k + 1, k + 1):
                    continue
                if split and T - 1 - k >= 2 and i == k + 2:
                    out += [(k, i, j, 0), (k, i, j, 1)]
                else:
                    out.append((k, i, j, -1))
    return out


def simulate(table, T, workers, selfl=True):
    """True when every task and chain step completes (no state in which every worker waits on a
    task nobody can run).  table: the claim order, claim index -> (k, i, j, h)."""
    ntasks = len(table)
    ver = {(i, j): 0 for i in range(T) for j in range(i + 1)}   # tile versions (steps applied)
    halves = {}
    lcnt = [0] * T   # panel row i's L published through step lcnt - 1
    bcnt = [0] * T   # b_i's updates through step bcnt - 1
    wdone = [False] * T
    d_next = 1       # the chain factors tile 0 itself first (the reducing form)
    wdone[0] = True
    nxt = 0
    held = [None] * workers

    def ready(t):
        k, i, j, h = t
        if j < 0:   # panel row i of step k
            return ver[(i, k)] >= k and bcnt[k] >= k and bcnt[i] >= k and wdone[k]
        if h >= 0 or (selfl and i == k + 2 and j >= k + 1):   # forms L_ik, L_jk itself
            return ver[(i, j)] >= k and ver[(i, k)] >= k and ver[(j, k)] >= k and wdone[k]
        return ver[(i, j)] >= k and lcnt[i] >= k + 1 and lcnt[j] >= k + 1

    def run(t):
        k, i, j, h = t
        if j < 0:
            lcnt[i] = k + 1
            bcnt[i] = k + 1
        elif h >= 0:
            halves[(i, j, k)] = halves.get((i, j, k), 0) + 1
            if halves[(i, j, k)] == 2:
                ver[(i, j)] = k + 1
        else:
            ver[(i, j)] = k + 1

    done = 0
    while done < ntasks or d_next < T:
        progress = False
        # the chain: step d needs tiles (d, d-1) and (d, d) through step d-2, and W_{d-1}
        if d_next < T and wdone[d_next - 1] and ver[(d_next, d_next - 1)] >= d_next - 1 and \
                ver[(d_next, d_next)] >= d_next - 1:
            ver[(d_next, d_next)] = d_next   # its own last update (the prepare)
            wdone[d_next] = True
            d_next += 1
            progress = True
        for w in range(workers):
            if held[w] is None and nxt < ntasks:
                held[w] = table[nxt]
                nxt += 1
                progress = True
            if held[w] is not None and ready(held[w]):
                run(held[w])
                held[w] = None
                done += 1
                progress = True
        if not progress:
            return False
    return True


@pytest.mark.parametrize("split,rowmajor", [(False, False), (True, False), (True, True), (False, True)])
def test_claim_order_is_a_permutation(claims, split, rowmajor):
    for T in range(2, 36):
        want = sorted(all_tasks(T, split))
        for order in (0, 1):
            assert sorted(claims.tables[(T, order, split, rowmajor)]) == want, (T, order)


@pytest.mark.parametrize("split,rowmajor", [(False, False), (True, False), (True, True), (False, True)])
def test_claim_orders_drain(claims, split, rowmajor):
    need = claims.need[split]   # order 1 needs more workers than one critical set holds
    for T in (2, 3, 4, 5, 8, 17, 33):
        for workers in (1, 2, 3, need - 1, need, need + 1, 16, 64):
            assert simulate(claims.tables[(T, 0, split, rowmajor)], T, workers), ("step order", T, workers)
            if workers >= need:
                assert simulate(claims.tables[(T, 1, split, rowmajor)], T, workers), ("order 1", T, workers)


def test_order1_needs_the_worker_guard(claims):
    """The model has teeth: with fewer workers than a critical set's waiting tasks order 1 stalls,
    and those are worker counts at which the kernel's guard (chol_claim_order) claims in step
    order."""
    assert not simulate(claims.tables[(8, 1, False, False)], 8, 3)
    assert not simulate(claims.tables[(8, 1, True, False)], 8, 5)
    assert claims.guard[False][3] == 0 and claims.need[False] > 3
    assert claims.guard[True][5] == 0 and claims.need[True] > 5
