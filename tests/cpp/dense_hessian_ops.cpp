// dense_hessian_ops.cpp -- replays a script of pnol::DenseInverseHessian operations
// (csrc/host/dense_hessian.hpp) on named objects and writes every result as raw doubles.
// All inputs and all expectations live in tests/test_gpu_dense_hessian.py; this program only
// replays.  Built against libpnol_amd.so with include/, csrc/ and csrc/host/ on the include path.
//
//   dense_hessian_ops <script> <results>
//
// Script (little-endian, packed): int32 count, then per operation int32 opcode, int32 id and
//   0 new        int32 n, int32 mode
//   1 child      int32 parent, int32 n, int32 mode          (the borrowing constructor)
//   2 drop
//   3 ident      int32 has_scale, [n doubles]
//   4 setmatrix  n * n doubles (row-major)
//   5 direction  n doubles g                                 -> p
//   6 update     int32 has_gnext, n doubles y, n doubles s, [n doubles gnext]   -> [pnext]
//   7 get                                                    -> n * n doubles
//   8 submatrix  int32 src, n int32 idx
//   9 exact?                                                 -> 1 double (0 / 1)
// Results: per operation double status (0 done, 1 the class threw std::runtime_error), double
// count, count doubles (count = 0 when it threw).  Anything else that goes wrong ends the
// program with a non-zero status.
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "dense_hessian.hpp"

namespace {

struct Fatal {
    std::string what;
};

struct Reader {
    FILE* f;
    int32_t i32() {
        int32_t v;
        if (std::fread(&v, sizeof v, 1, f) != 1) throw Fatal{"script truncated (int32)"};
        return v;
    }
    std::vector<double> doubles(size_t count) {
        std::vector<double> v(count);
        if (count && std::fread(v.data(), sizeof(double), count, f) != count) throw Fatal{"script truncated (doubles)"};
        return v;
    }
};

struct Writer {
    FILE* f;
    void record(bool threw, const std::vector<double>& payload) {
        const double head[2] = {threw ? 1.0 : 0.0, threw ? 0.0 : (double)payload.size()};
        if (std::fwrite(head, sizeof(double), 2, f) != 2) throw Fatal{"result write failed"};
        if (!threw && !payload.empty() &&
            std::fwrite(payload.data(), sizeof(double), payload.size(), f) != payload.size())
            throw Fatal{"result write failed"};
    }
};

typedef pnol::DenseInverseHessian Hess;

struct Objects {
    std::map<int, std::unique_ptr<Hess>> byId;
    std::vector<int> order;   // creation order: a reduced D must go before the D it borrows from
    Hess& at(int id) {
        auto it = byId.find(id);
        if (it == byId.end()) throw Fatal{"unknown object id " + std::to_string(id)};
        return *it->second;
    }
    void add(int id, Hess* h) {
        std::unique_ptr<Hess> p(h);
        if (byId.count(id)) throw Fatal{"object id " + std::to_string(id) + " used twice"};
        byId[id] = std::move(p);
        order.push_back(id);
    }
    void drop(int id) {
        if (!byId.erase(id)) throw Fatal{"unknown object id " + std::to_string(id)};
    }
    ~Objects() {
        for (size_t k = order.size(); k-- > 0;) byId.erase(order[k]);
    }
};

// a std::runtime_error of the class is a result ("threw"); the run goes on
template <class F>
bool threwIn(int k, F&& call) {
    try {
        call();
        return false;
    } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "op %d threw: %s\n", k, e.what());
        return true;
    }
}

void replay(pnol_ctx* ctx, Reader& in, Writer& out) {
    Objects objs;
    const int count = in.i32();
    for (int k = 0; k < count; ++k) {
        const int op = in.i32(), id = in.i32();
        std::vector<double> payload;
        bool threw = false;
        // every operand is read before the class is called, so a throw leaves the script in step
        switch (op) {
        case 0: {
            const int n = in.i32(), mode = in.i32();
            threw = threwIn(k, [&] { objs.add(id, new Hess(ctx, n, mode)); });
            break;
        }
        case 1: {
            const int parent = in.i32(), n = in.i32(), mode = in.i32();
            Hess& p = objs.at(parent);
            threw = threwIn(k, [&] { objs.add(id, new Hess(p, n, mode)); });
            break;
        }
        case 2:
            objs.drop(id);
            break;
        case 3: {
            Hess& h = objs.at(id);
            const int has = in.i32();
            std::vector<double> scale = in.doubles(has ? (size_t)h.n() : 0);
            threw = threwIn(k, [&] { h.setIdentity(has ? &scale : nullptr); });
            break;
        }
        case 4: {
            Hess& h = objs.at(id);
            const int n = h.n();
            std::vector<double> flat = in.doubles((size_t)n * n);
            std::vector<std::vector<double>> M(n, std::vector<double>(n));
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) M[i][j] = flat[(size_t)i * n + j];
            threw = threwIn(k, [&] { h.setMatrix(M); });
            break;
        }
        case 5: {
            Hess& h = objs.at(id);
            std::vector<double> g = in.doubles((size_t)h.n());
            threw = threwIn(k, [&] { h.direction(g, payload); });
            break;
        }
        case 6: {
            Hess& h = objs.at(id);
            const int has = in.i32();
            std::vector<double> y = in.doubles((size_t)h.n()), s = in.doubles((size_t)h.n());
            std::vector<double> g = in.doubles(has ? (size_t)h.n() : 0);
            threw = threwIn(k, [&] { h.update(y, s, has ? &g : nullptr, has ? &payload : nullptr); });
            break;
        }
        case 7: {
            Hess& h = objs.at(id);
            std::vector<std::vector<double>> M;
            threw = threwIn(k, [&] { h.getMatrix(M); });
            for (const std::vector<double>& row : M) payload.insert(payload.end(), row.begin(), row.end());
            break;
        }
        case 8: {
            Hess& h = objs.at(id);
            Hess& src = objs.at(in.i32());
            std::vector<int> idx((size_t)h.n());
            for (int& v : idx) v = in.i32();
            threw = threwIn(k, [&] { h.setSubmatrixOf(src, idx); });
            break;
        }
        case 9:
            payload.push_back(objs.at(id).exact() ? 1.0 : 0.0);
            break;
        default:
            throw Fatal{"unknown opcode " + std::to_string(op)};
        }
        out.record(threw, payload);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <script> <results>\n", argv[0]);
        return 2;
    }
    FILE* fin = std::fopen(argv[1], "rb");
    FILE* fout = fin ? std::fopen(argv[2], "wb") : nullptr;
    if (!fin || !fout) {
        std::fprintf(stderr, "cannot open %s\n", fin ? argv[2] : argv[1]);
        return 2;
    }
    pnol_ctx* ctx = nullptr;
    if (pnol_ctx_create(0, &ctx) != PNOL_OK || !ctx) {
        std::fprintf(stderr, "pnol_ctx_create(0) failed: no gfx950 device visible\n");
        return 3;
    }
    int rc = 0;
    try {
        Reader in{fin};
        Writer out{fout};
        replay(ctx, in, out);
    } catch (const Fatal& e) {
        std::fprintf(stderr, "dense_hessian_ops: %s\n", e.what.c_str());
        rc = 4;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "dense_hessian_ops: unexpected %s\n", e.what());
        rc = 5;
    }
    pnol_ctx_destroy(ctx);
    if (std::fclose(fout) != 0) rc = rc ? rc : 6;
    std::fclose(fin);
    return rc;
}
