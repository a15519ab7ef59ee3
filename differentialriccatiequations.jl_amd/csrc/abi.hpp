// What the translation units of the C ABI share (api.hip, api_lowrank.hip, api_dense.hip, api_probe.hip): the handle structs behind the opaque
// types of include/dre_hip.h, guarded(), the row-order and download helpers, and the member helpers of the batched calls.  Private to csrc/.
#pragma once
#include "../../include/dre_hip.h"

#include <map>
#include <string>
#include <vector>

#include "abi_out.hpp"
#include "dense_batch.hpp"
#include "dense_sylvester.hpp"
#include "engine.hpp"
#include "profiling.hpp"

struct dre_ctx { dre::Ctx c; std::map<std::string, dre::KernelStat> merged; std::vector<std::string> batch_errors; };
struct dre_dense { dre::Mat m; };
struct dre_pencil {
    std::unique_ptr<dre::Pencil> p;
    std::vector<double> hE, hA;
};
struct dre_factor {
    const dre_pencil* pen = nullptr;
    bool is_cplx = false;
    dre::Factor<double> fr;
    dre::Factor<dre::cplx> fc;
};
struct dre_ldlt {
    dre::LDLtP x;
    const dre_pencil* pen = nullptr;
};
struct dre_adi_result {
    dre::AdiResult r;
    const dre_pencil* pen = nullptr;
};
struct dre_gdre_result {
    dre::GdreResult r;
    const dre_pencil* pen = nullptr;
    int m = 0;
    // dense path (dre_dense_gdre_solve): pen is null, K(t) lives in r.Kt, the states and per-solve statistics here
    bool dense = false;
    int n = 0;
    std::vector<dre::Mat> Xd;
    std::vector<dre::SignStats> solves;
    // adaptive dense path (dre_dense_gdre_solve_adaptive): trial steps accepted / rejected, the error measure of every accepted step
    bool adaptive = false;
    int64_t accepted = 0, rejected = 0;
    std::vector<double> step_err;
};

struct dre_sign { std::unique_ptr<dre::SignLyap> s; };
struct dre_sylvester { std::unique_ptr<dre::SignSylvester> s; };

namespace dre {

extern thread_local std::string g_noctx_error;          // dre_last_error(nullptr); defined in api.hip

template <typename F>
int guarded(dre_ctx* ctx, F&& f) {
    try {
        f();
        return DRE_OK;
    } catch (const Error& e) {
        if (ctx) ctx->c.last_error = e.what(); else g_noctx_error = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        if (ctx) ctx->c.last_error = "out of host memory";
        return DRE_ERR_ALLOC;
    } catch (const std::exception& e) {
        if (ctx) ctx->c.last_error = e.what(); else g_noctx_error = e.what();
        return DRE_ERR_INTERNAL;
    }
}

// an entry point that returns handles of type H: f gets their owner (abi_out.hpp), which commits once f has returned without throwing
template <typename H, typename F>
int guarded_out(dre_ctx* ctx, F&& f) {
    return guarded(ctx, [&] { AbiOut<H> o; f(o); o.commit(); });
}
// the dense results: one way to make a handle that holds m
using DenseOut = AbiOut<dre_dense>;
inline dre_dense* put(DenseOut& o, dre_dense** slot, Mat m) {
    dre_dense* h = o.make(slot);
    h->m = std::move(m);
    return h;
}
inline void put(AbiOut<dre_ldlt>& o, dre_ldlt** slot, LDLtP x, const dre_pencil* pen) {
    dre_ldlt* h = o.make(slot);
    h->x = std::move(x); h->pen = pen;
}
// the optional operand of a dense call: a null handle is the solver's default
inline const Mat* opt_mat(const dre_dense* h) { return h ? &h->m : nullptr; }

inline void download_mat(Ctx* c, const Mat& m, double* host, int ld) {
    DRE_REQUIRE(ld >= std::max(m.rows, 1), "download: leading dimension too small");
    if (m.rows > 0 && m.cols > 0) {
        DRE_HIP(hipMemcpy2DAsync(host, (size_t)ld * sizeof(double), m.p, (size_t)m.ld * sizeof(double),
                                 (size_t)m.rows * sizeof(double), m.cols, hipMemcpyDeviceToHost, c->stream));
    }
    DRE_HIP(hipStreamSynchronize(c->stream));
}
// rows of user-ordered matrices <-> solver ordering
inline Mat to_solver_order(Ctx* c, const dre_pencil* pen, const Mat& src) {
    if (!pen) return src;
    DRE_REQUIRE(src.rows == pen->p->n, "matrix row count does not match the pencil");
    Mat dst(c, src.rows, src.cols);
    permute_rows(c, src, pen->p->perm.p, dst);     // dst(new,:) = src(perm[new],:)
    return dst;
}
inline Mat to_user_order(Ctx* c, const dre_pencil* pen, const Mat& src) {
    if (!pen) return src;
    Mat dst(c, src.rows, src.cols);
    permute_rows(c, src, pen->p->iperm.p, dst);    // dst(old,:) = src(iperm[old],:)
    return dst;
}

// ---- the batched calls: member handles -> one stack (rows x cols*batch, member b at b * rows * cols) ----------------------------------
inline Mat pack_stack(Ctx* c, int batch, const dre_dense* const* h, int rows, int cols) {
    Mat S(c, rows, cols * batch);
    for (int b = 0; b < batch; ++b) {
        Mat v = S.colsview(b * cols, cols);
        copy_mat(c, h[b]->m, v);
    }
    return S;
}
inline void check_members(int batch, const dre_dense* const* h, int rows, int cols, const char* who, const char* what) {
    for (int b = 0; b < batch; ++b)
        DRE_REQUIRE(h[b] && h[b]->m.rows == rows && h[b]->m.cols == cols, std::string(who) + ": " + what + " of member " + std::to_string(b) + " must be " +
                                                                              std::to_string(rows) + " x " + std::to_string(cols));
}
inline void check_batch_order(int batch, int n, const char* who) {
    DRE_REQUIRE(batch >= 1 && batch <= 65535, std::string(who) + ": batch must be in 1 .. 65535");
    DRE_REQUIRE(n >= 1 && n <= GJ_REGISTER_MAX_N, std::string(who) + ": the batched dense path inverts with the register panel, order 1 .. " +
                                                      std::to_string(GJ_REGISTER_MAX_N) + " (n = " + std::to_string(n) + ")");
}
inline std::vector<Mat> member_mats(int batch, const dre_dense* const* h, const char* who, const char* what) {
    std::vector<Mat> v((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        DRE_REQUIRE(h[b], std::string(who) + ": " + what + " of member " + std::to_string(b) + " is null");
        v[(size_t)b] = h[b]->m;
    }
    return v;
}
// per-member outcomes -> status[], the context's per-member messages, dre_last_error = the first failed member's
inline void report_members(dre_ctx* ctx, const std::vector<BatchMemberStatus>& st, int32_t* status) {
    ctx->batch_errors.assign(st.size(), std::string());
    bool first = true;
    for (size_t b = 0; b < st.size(); ++b) {
        if (status) status[b] = st[b].code;
        if (!st[b].code) continue;
        ctx->batch_errors[b] = st[b].msg;
        if (first) { ctx->c.last_error = st[b].msg; first = false; }
    }
}

}  // namespace dre
