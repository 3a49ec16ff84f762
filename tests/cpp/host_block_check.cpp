// host_block_check.cpp -- the device-block layout of the host-pointer batched calls
// (csrc/host_block.hpp) on the array lists capi.cpp passes, optional arrays present and absent.
// Built with -fsanitize=address,undefined by tests/test_host_block.py; no device, no HIP.
// Every array's bytes are written at its offset in a block of exactly the returned size, so an
// offset past the end or a misaligned 8-byte item is a sanitizer report; overlap, alignment and
// the total are also checked by hand.  Exit 0 = clean.
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_block.hpp"

using namespace pnol;

static int check(const char* name, const std::vector<HostArray>& a) {
    std::vector<size_t> off(a.size());
    const size_t total = host_block_carve(a.data(), a.size(), off.data());
    size_t sum = 0;
    for (const HostArray& h : a) sum += h.bytes();
    if (total != sum) return std::printf("%s: total %zu, parts %zu\n", name, total, sum), 1;
    std::vector<unsigned char> owner(total, 0xff);
    char* block = new char[total];   // exactly `total`: the sanitizer sees one byte too many
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i].elem == 8 && off[i] % 8 != 0) return std::printf("%s: array %zu at %zu\n", name, i, off[i]), 1;
        if (a[i].elem == 4 && off[i] % 4 != 0) return std::printf("%s: array %zu at %zu\n", name, i, off[i]), 1;
        for (size_t k = 0; k < a[i].bytes(); ++k) {
            unsigned char& own = owner[off[i] + k];
            if (own != 0xff) return std::printf("%s: arrays %zu and %d overlap\n", name, i, own), 1;
            own = (unsigned char)i;
        }
        for (size_t k = 0; k < (a[i].host ? a[i].count : 0); ++k) {
            if (a[i].elem == 8) reinterpret_cast<double*>(block + off[i])[k] = (double)i;
            else reinterpret_cast<int*>(block + off[i])[k] = (int)i;
        }
    }
    delete[] block;
    // the 8-byte items come first, each group in list order
    size_t at = 0;
    for (int wide = 1; wide >= 0; --wide)
        for (size_t i = 0; i < a.size(); ++i)
            if ((a[i].elem == 8) == (wide == 1)) {
                if (off[i] != at) return std::printf("%s: array %zu at %zu, expected %zu\n", name, i, off[i], at), 1;
                at += a[i].bytes();
            }
    return 0;
}

int main() {
    double d;
    void* h = &d;   // any non-null host pointer: the layout never reads through it
    int bad = 0;
    for (size_t np : {1, 3, 63, 64, 65, 130})
        for (size_t m : {1, 4, 33})
            for (int f = 0; f < 4; ++f) {
                const size_t nm = np * m;
                // pnol_run_levmarq_batch: y, X, chi0, chi, evals, iters, F0, FOpt (n = 3)
                void *F0 = f & 1 ? h : nullptr, *FOpt = f & 2 ? h : nullptr;
                bad += check("levmarq", {{h, nm, 8, kHostIn}, {h, np * 3, 8, kHostIn | kHostOut}, {h, np, 8, kHostOut},
                                         {h, np, 8, kHostOut}, {h, np, 8, kHostOut}, {h, np, 4, kHostOut},
                                         {F0, nm, 8, kHostOut}, {FOpt, nm, 8, kHostOut}});
            }
    for (size_t ns : {1, 3, 63, 64, 65, 130})
        for (size_t n : {1, 5, 12}) {
            // pnol_run_simplex_batch: X, f0, fopt, evals, iters
            bad += check("simplex", {{h, ns * n, 8, kHostIn | kHostOut}, {h, ns, 8, kHostOut}, {h, ns, 8, kHostOut},
                                     {h, ns, 8, kHostOut}, {h, ns, 4, kHostOut}});
            // pnol_run_bfgs_batch: X, f0, fopt, gnorm, evals, iters
            bad += check("bfgs", {{h, ns * n, 8, kHostIn | kHostOut}, {h, ns, 8, kHostOut}, {h, ns, 8, kHostOut},
                                  {h, ns, 8, kHostOut}, {h, ns, 8, kHostOut}, {h, ns, 4, kHostOut}});
        }
    // an int array listed before 8-byte ones with an odd count: the wide items still come first
    bad += check("mixed", {{h, 3, 4, kHostOut}, {h, 5, 8, kHostIn}, {nullptr, 7, 8, kHostOut}, {h, 1, 4, kHostOut},
                           {h, 2, 8, kHostOut}});
    if (bad) return 1;
    std::printf("host_block_check: clean\n");
    return 0;
}
