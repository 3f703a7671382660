// What the two product forms of MuonAdamAtan2 share: the device description of a matrix, the plan and its table builder.
// csrc/muon.hip holds the fp32 form (products 0), the entry points and the multi-tensor kernels; csrc/muon_bf16.hip the bf16 form (products 1).
//
// Work-buffer layout of one matrix, in 4-byte units from the start of the pass's work buffer:
//   products 0   x0, x1: X and X' (Rp x Cp floats each);  a, b: A and B (Rp x Rp floats each)
//   products 1   x0, x1: two regions of Rp x Cp floats.  Each holds a bf16 X [Rp][Cp] followed by its transposed image X^T [Cp][Rp]; the region at x0 is
//                first the fp32 image of u that prepare writes (normalise reads it into the region at x1, iteration 0's apply is the first to overwrite it);
//                a, b: bf16 A and B [Rp][Rp] (Rp x Rp / 2 units each)
#pragma once
#include <string.h>
#include <vector>

#include "../../include/d4hip.h"
#include "common.h"

namespace d4 {

constexpr int MU_T = 128;             // output tile of a workgroup, and the padding unit of every work-buffer dimension
constexpr int MU_STRIP = 32;          // rows of the original matrix per prepare / finish workgroup

struct MuonMat {                      // one matrix of a pass (device table)
    float* w;                         // parameter (null: d4_newton_schulz, `out` is written without a read)
    const float* g;                   // gradient / input
    float* m;                         // momentum (null: u = g)
    float* out;                       // destination of finish (== w for the optimiser)
    int r, c;                         // shape as given
    int R, C;                         // oriented: R = min(r, c) rows
    int Rp, Cp;                       // padded to MU_T
    int transposed;                   // r > c
    int part0;                        // first partial of this matrix
    int nparts;                       // strips (partials) of this matrix
    float coef;                       // finish: out = decay * w + coef * X
    int64_t x0, x1, a, b;             // float offsets of X, X', A, B in the pass's work buffer
};

}  // namespace d4

struct d4_muon_plan {
    struct Pass {
        int first, count;                            // matrices [first, first + count)
        int n_prep, n_sym, n_full;                   // workgroups of prepare / finish, of the symmetric stages, of the apply stage
        size_t prep_off, sym_off, full_off;          // byte offsets in `tables`
        size_t work_floats;
    };
    std::vector<d4::MuonMat> mats;                   // host image (pointers filled per call)
    std::vector<Pass> passes;
    std::vector<const void*> last;                   // pointers of the last upload (4 per matrix)
    std::vector<float> last_coef;
    char* tables = nullptr;                          // device: [MuonMat x n][per pass: prepare blocks, symmetric tiles, apply tiles]
    size_t work_bytes = 0, part_floats = 0;
    bool uploaded = false;
    int products = 0;                                // 0: fp32 products (csrc/muon.hip), 1: bf16 products (csrc/muon_bf16.hip)
};

namespace d4 {

// the bf16 form's launches (csrc/muon_bf16.hip); the sequence of a call is muon_run's (csrc/muon.hip): per pass  prepare (the fp32 form's own kernel),
// normalise, steps x (gram, poly, apply), finish.  `cur` is the region that holds X: 0 the one at x1, 1 the one at x0.
int muon_bf16_normalise(const MuonMat* mats, const int2* blocks, int nblocks, float* work, const float* partials, float eps, hipStream_t s);
int muon_bf16_product(const MuonMat* mats, const int4* tiles, int ntiles, float* work, int stage, int cur, float alpha, float beta, hipStream_t s);
int muon_bf16_finish(const MuonMat* mats, const int2* blocks, int nblocks, const float* work, int cur, float decay, hipStream_t s);

// passes, work-buffer offsets and the device tables of a group; `who` names the entry point in refusals
static inline int muon_plan_build(const char* who, int n, const int32_t* rows, const int32_t* cols, size_t workspace_bytes, int products, d4_muon_plan** out) {
    D4_REQUIRE(out, "%s: out is null", who);
    *out = nullptr;
    D4_REQUIRE(products == 0 || products == 1, "%s: products = %d (0: fp32, 1: bf16)", who, products);
    D4_REQUIRE(n >= 1 && rows && cols, "%s: n >= 1, rows and cols", who);
    auto* pl = new d4_muon_plan;
    pl->products = products;
    pl->mats.resize(n);
    pl->last.assign(4 * (size_t)n, nullptr);
    pl->last_coef.assign(n, 0.f);
    auto fail = [&]() { delete pl; return 2; };
    auto pad = [](int v) { return (v + MU_T - 1) / MU_T * MU_T; };
    int part = 0;
    d4_muon_plan::Pass cur{0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int2> prep;
    std::vector<int4> sym, full;
    struct Built { std::vector<int2> prep; std::vector<int4> sym, full; };
    std::vector<Built> built;
    auto close = [&]() {
        cur.n_prep = (int)prep.size(); cur.n_sym = (int)sym.size(); cur.n_full = (int)full.size();
        pl->passes.push_back(cur);
        built.push_back(Built{prep, sym, full});
        if (cur.work_floats * 4 > pl->work_bytes) pl->work_bytes = cur.work_floats * 4;
        prep.clear(); sym.clear(); full.clear();
    };
    for (int i = 0; i < n; ++i) {
        if (!(rows[i] >= 1 && cols[i] >= 1)) { set_error("%s: matrix %d has rows = %d, cols = %d (both must be >= 1)", who, i, rows[i], cols[i]); return fail(); }
        if (!(rows[i] <= (1 << 20) && cols[i] <= (1 << 20))) { set_error("%s: matrix %d: rows = %d, cols = %d exceed 2^20", who, i, rows[i], cols[i]); return fail(); }
        MuonMat& d = pl->mats[i];
        memset(&d, 0, sizeof(d));
        d.r = rows[i]; d.c = cols[i];
        d.transposed = d.r > d.c;
        d.R = d.transposed ? d.c : d.r; d.C = d.transposed ? d.r : d.c;
        d.Rp = pad(d.R); d.Cp = pad(d.C);
        const int rp_o = d.transposed ? d.Cp : d.Rp;                     // padded rows of the original orientation
        d.nparts = rp_o / MU_STRIP; d.part0 = part; part += d.nparts;
        const size_t xsz = (size_t)d.Rp * d.Cp;                          // products 1: bf16 X and X^T together
        const size_t asz = products ? (size_t)d.Rp * d.Rp / 2 : (size_t)d.Rp * d.Rp;
        const size_t need = 2 * xsz + 2 * asz;
        if (need * 4 > workspace_bytes) {
            set_error("%s: matrix %d (%d x %d) needs %zu bytes of work buffers, workspace_bytes is %zu", who, i, d.r, d.c, need * 4, workspace_bytes);
            return fail();
        }
        if (cur.count > 0 && (cur.work_floats + need) * 4 > workspace_bytes) { close(); cur = d4_muon_plan::Pass{i, 0, 0, 0, 0, 0, 0, 0, 0}; }
        size_t at = cur.work_floats;
        d.x0 = (int64_t)at; at += xsz;
        d.x1 = (int64_t)at; at += xsz;
        d.a = (int64_t)at; at += asz;
        d.b = (int64_t)at; at += asz;
        cur.work_floats = at; cur.count++;
        for (int sidx = 0; sidx < d.nparts; ++sidx) prep.push_back(make_int2(i, sidx));
        const int tm = d.Rp / MU_T, tn = d.Cp / MU_T;
        for (int y = 0; y < tm; ++y)
            for (int x = y; x < tm; ++x) sym.push_back(make_int4(i, y, x, 0));
        for (int y = 0; y < tm; ++y)
            for (int x = 0; x < tn; ++x) full.push_back(make_int4(i, y, x, 0));
    }
    close();
    pl->part_floats = (size_t)part;
    // device tables
    size_t bytes = (sizeof(MuonMat) * (size_t)n + 15) & ~(size_t)15;
    for (size_t k = 0; k < built.size(); ++k) {
        auto& ps = pl->passes[k];
        ps.prep_off = bytes; bytes += (built[k].prep.size() * sizeof(int2) + 15) & ~(size_t)15;
        ps.sym_off = bytes; bytes += built[k].sym.size() * sizeof(int4);
        ps.full_off = bytes; bytes += built[k].full.size() * sizeof(int4);
    }
    std::vector<char> host(bytes, 0);
    for (size_t k = 0; k < built.size(); ++k) {
        const auto& ps = pl->passes[k];
        memcpy(host.data() + ps.prep_off, built[k].prep.data(), built[k].prep.size() * sizeof(int2));
        memcpy(host.data() + ps.sym_off, built[k].sym.data(), built[k].sym.size() * sizeof(int4));
        memcpy(host.data() + ps.full_off, built[k].full.data(), built[k].full.size() * sizeof(int4));
    }
    hipError_t e = hipMalloc((void**)&pl->tables, bytes);
    if (e == hipSuccess) e = hipMemcpy(pl->tables, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (pl->tables) (void)hipFree(pl->tables);
        delete pl;
        return hip_fail(e, "d4_muon_plan_create: device tile table");
    }
    *out = pl;
    return 0;
}

}  // namespace d4
