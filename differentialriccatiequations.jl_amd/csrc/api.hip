#include <functional>
// C ABI of libdre_hip (declared in include/dre_hip.h).
#include "../../include/dre_hip.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <limits>

#include "balance.hpp"
#include "comm.hpp"
#include "dense_adaptive.hpp"
#include "dense_are.hpp"
#include "dense_are_batch.hpp"
#include "dense_batch.hpp"
#include "dense_doubling.hpp"
#include "dense_gj.hpp"
#include "dense_sign.hpp"
#include "dense_sign_lr.hpp"
#include "dense_sylvester.hpp"
#include "engine.hpp"
#include "dense_cgj.hpp"
#include "freq_response.hpp"
#include "time_response.hpp"
#include "transfer_eval.hpp"
#include "gemm_probe_check.hpp"
#include "hostla.hpp"
#include "jacobi_batch.hpp"
#include "profiling.hpp"
#include "svd_jacobi.hpp"
#include "sym_jacobi.hpp"

using namespace dre;

struct dre_ctx { Ctx c; std::map<std::string, KernelStat> merged; std::vector<std::string> batch_errors; };
struct dre_dense { Mat m; };
struct dre_pencil {
    std::unique_ptr<Pencil> p;
    std::vector<double> hE, hA;
};
struct dre_factor {
    const dre_pencil* pen = nullptr;
    bool is_cplx = false;
    Factor<double> fr;
    Factor<cplx> fc;
};
struct dre_ldlt {
    LDLtP x;
    const dre_pencil* pen = nullptr;
};
struct dre_adi_result {
    AdiResult r;
    const dre_pencil* pen = nullptr;
};
struct dre_gdre_result {
    GdreResult r;
    const dre_pencil* pen = nullptr;
    int m = 0;
    // dense path (dre_dense_gdre_solve): pen is null, K(t) lives in r.Kt, the states and per-solve statistics here
    bool dense = false;
    int n = 0;
    std::vector<Mat> Xd;
    std::vector<SignStats> solves;
    // adaptive dense path (dre_dense_gdre_solve_adaptive): trial steps accepted / rejected, the error measure of every accepted step
    bool adaptive = false;
    int64_t accepted = 0, rejected = 0;
    std::vector<double> step_err;
};

struct dre_sign { std::unique_ptr<SignLyap> s; };
struct dre_sylvester { std::unique_ptr<SignSylvester> s; };

static thread_local std::string g_noctx_error;

template <typename F>
static int guarded(dre_ctx* ctx, F&& f) {
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

extern "C" {

int dre_version(void) { return 120; }  // 101: dense path (dre_dense_gale_solve, dre_dense_gdre_solve); 102: dre_dense_invert, dense_gj_panel, n > 4096;
                                        // 103: dense GARE (dre_dense_gare_solve, dre_dense_gare_residual); 104: factored sign solver (dre_sign_*); 105: batched dense path (dre_dense_*_batched);
                                        // 106: batched dense GARE (dre_dense_gare_solve_batched); 107: adaptive dense Ros2 (dre_dense_gdre_solve_adaptive,
                                        // dre_gdre_result_step_stats, DRE_ERR_STEP); 108: dre_gemm_probe (test surface of the GEMM family), gemm_swizzle = 2;
                                        // 109: dual solves on a kept sign factorisation (dre_sign_solve_dense_t, dre_sign_solve_lr_t);
                                        // 110: device SVD and balanced truncation (dre_svd_jacobi, dre_balance_lr)
                                        // 111: batched block Jacobi and ensemble balanced truncation (dre_sym_eig_jacobi_batched, dre_svd_jacobi_batched,
                                        //      dre_balance_lr_batched)
                                        // 112: frequency response batched by frequency (dre_freq_response, dre_freq_response_batched)
                                        // 113: LQG balanced truncation from one Hamiltonian sign iteration (dre_dense_gare_solve_pair, dre_lqg_balance)
                                        // 114: dre_sym_eig_probe (test surface of the Householder + QL eigensolver); sym_eig refuses a non-finite input
                                        // 115: complex Gauss-Jordan inversion and the transfer function at complex points (dre_dense_invert_complex_batched,
                                        //      dre_transfer_eval, dre_transfer_eval_batched)
                                        // 116: dre_adi_chain_probe (test surface of the dense-inverse ADI chain)
                                        // 117: time response of dense descriptor systems: step, impulse, simulate (dre_time_response)
                                        // 118: discrete-time dense solvers by doubling: Stein and DARE (dre_dense_stein_solve, dre_dense_stein_residual,
                                        //      dre_dense_dare_solve, dre_dense_dare_solve_pair, dre_dense_dare_residual)
                                        // 119: dense generalized Sylvester solver by the coupled sign iteration (dre_dense_sylvester_solve,
                                        //      dre_dense_sylvester_residual, dre_sylvester_create, dre_sylvester_solve, dre_sylvester_iters,
                                        //      dre_sylvester_destroy)
                                        // 120: dre_warm_probe (test surface of the warm-started compression, warm.hip)

int dre_ctx_create(int device, dre_ctx** out) {
    if (!out) return DRE_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_noctx_error = "no usable HIP device (libdre_hip has no CPU fallback)";
        return DRE_ERR_NODEVICE;
    }
    if (device < 0 || device >= ndev) { g_noctx_error = "device index out of range"; return DRE_ERR_INVALID; }
    auto* ctx = new dre_ctx();
    int rc = guarded(ctx, [&] {
        DRE_HIP(hipSetDevice(device));
        ctx->c.device = device;
        ctx->c.stream = create_stream(0);
        hipDeviceProp_t prop;
        DRE_HIP(hipGetDeviceProperties(&prop, device));
        ctx->c.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        ctx->c.timer = std::make_unique<KernelTimer>();
    });
    if (rc != DRE_OK) { g_noctx_error = ctx->c.last_error; delete ctx; return rc; }
    // DRE_OPTIONS="name=value,name=value": the options of dre_ctx_set_option for every context of the process (tools/option_matrix.sh runs
    // the test suite under each configuration this way); an unknown name is an error like in the call
    if (const char* e = std::getenv("DRE_OPTIONS")) {
        std::string all = e;
        size_t pos = 0;
        while (pos < all.size()) {
            size_t end = all.find(',', pos);
            if (end == std::string::npos) end = all.size();
            const std::string item = all.substr(pos, end - pos);
            pos = end + 1;
            // (a typo must not run the default configuration and report green: "name:0", "name=off", "name = 1x" are errors)
            auto trim = [](std::string t) { const size_t a0 = t.find_first_not_of(" \t"); if (a0 == std::string::npos) return std::string(); return t.substr(a0, t.find_last_not_of(" \t") - a0 + 1); };
            const std::string it2 = trim(item);
            if (it2.empty()) continue;
            const size_t eq = it2.find('=');
            int rc2 = DRE_OK;
            if (eq == std::string::npos || eq == 0) { ctx->c.last_error = "item '" + it2 + "' is not of the form name=value"; rc2 = DRE_ERR_INVALID; }
            else {
                const std::string nm = trim(it2.substr(0, eq)), vs = trim(it2.substr(eq + 1));
                char* endp = nullptr;
                const double v = std::strtod(vs.c_str(), &endp);
                if (vs.empty() || endp == vs.c_str() || *endp != '\0') { ctx->c.last_error = "item '" + it2 + "': '" + vs + "' is not a number"; rc2 = DRE_ERR_INVALID; }
                else rc2 = dre_ctx_set_option(ctx, nm.c_str(), v);
            }
            if (rc2 != DRE_OK) { g_noctx_error = "DRE_OPTIONS: " + ctx->c.last_error; dre_ctx_destroy(ctx); return rc2; }
        }
    }
    *out = ctx;
    return DRE_OK;
}
int dre_ctx_destroy(dre_ctx* ctx) {
    if (!ctx) return DRE_OK;
    (void)hipSetDevice(ctx->c.device);
    (void)hipStreamSynchronize(ctx->c.stream);
    for (auto& w : ctx->c.parked_worker) w.reset();          // (parked: they hold no job between solves; joined here, before their streams go)
    ctx->c.comm.reset();
    if (ctx->c.side) {
        Ctx& sc = *ctx->c.side;
        (void)hipStreamSynchronize(sc.stream);
        for (size_t h = 0; h < sc.helpers.size(); ++h) {
            Ctx& hc = *sc.helpers[h];
            (void)hipStreamSynchronize(hc.stream);
            hc.timer.reset(); hc.pool.trim();
            (void)hipEventDestroy(sc.helper_ev[h]);
            (void)hipStreamDestroy(hc.stream);
        }
        sc.helpers.clear(); sc.helper_ev.clear();
        if (sc.helper_e0) { (void)hipEventDestroy(sc.helper_e0); sc.helper_e0 = nullptr; }
        sc.timer.reset(); sc.pool.trim();
        if (sc.fetch_host) { (void)hipHostFree((void*)sc.fetch_host); sc.fetch_host = nullptr; }
        (void)hipEventDestroy(ctx->c.side_e1); (void)hipEventDestroy(ctx->c.side_e2);
        (void)hipStreamDestroy(sc.stream);
        ctx->c.side.reset();
    }
    auto drop_helpers = [](Ctx& owner) {
        for (size_t h = 0; h < owner.helpers.size(); ++h) {
            Ctx& hc = *owner.helpers[h];
            (void)hipStreamSynchronize(hc.stream);
            hc.timer.reset(); hc.pool.trim();
            if (hc.fetch_host) { (void)hipHostFree((void*)hc.fetch_host); hc.fetch_host = nullptr; }
            (void)hipEventDestroy(owner.helper_ev[h]);
            (void)hipStreamDestroy(hc.stream);
        }
        owner.helpers.clear(); owner.helper_ev.clear();
        if (owner.helper_e0) { (void)hipEventDestroy(owner.helper_e0); owner.helper_e0 = nullptr; }
        for (auto& e : owner.aux_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    };
    drop_helpers(ctx->c);
    ctx->c.timer.reset();
    ctx->c.pool.trim();
    if (ctx->c.fetch_host) { (void)hipHostFree((void*)ctx->c.fetch_host); ctx->c.fetch_host = nullptr; }
    if (ctx->c.dense_land) { (void)hipHostFree(ctx->c.dense_land); ctx->c.dense_land = nullptr; }
    (void)hipStreamDestroy(ctx->c.stream);
    delete ctx;
    return DRE_OK;
}
const char* dre_last_error(dre_ctx* ctx) { return ctx ? ctx->c.last_error.c_str() : g_noctx_error.c_str(); }
int dre_ctx_sync(dre_ctx* ctx) { return guarded(ctx, [&] { ctx->c.sync(); }); }
int dre_ctx_info(dre_ctx* ctx, int64_t* info) {
    info[0] = ctx->c.num_cus; info[1] = (int64_t)ctx->c.pool.total_bytes();
    return DRE_OK;
}
// One table for dre_ctx_set_option / dre_ctx_get_option / DRE_OPTIONS: the option's storage by name (exactly one of i / d is set)
struct OptionRef { int* i = nullptr; double* d = nullptr; };
static OptionRef option_ref(Ctx& c, const std::string& key) {
    OptionRef r;
#define DRE_OPT_I(NAME, FIELD) if (key == NAME) { r.i = &c.FIELD; return r; }
#define DRE_OPT_D(NAME, FIELD) if (key == NAME) { r.d = &c.FIELD; return r; }
    DRE_OPT_I("dense_inverse_max_n", dense_inv_max_n)
    DRE_OPT_I("compress_direct_max_n", compress_direct_max_n)
    DRE_OPT_D("compress_direct_ratio", compress_direct_ratio)
    DRE_OPT_I("compress_factor_min_n", compress_factor_min_n)
    DRE_OPT_I("compress_factor_min_cols", compress_factor_min_cols)
    DRE_OPT_I("compress_sketch", compress_sketch)
    DRE_OPT_I("compress_sketch_min_cols", compress_sketch_min_cols)
    DRE_OPT_I("compress_sketch_extra", compress_sketch_extra)
    DRE_OPT_I("compress_sketch_cholqr", compress_sketch_cholqr)
    DRE_OPT_I("compress_sketch_sparse", compress_sketch_sparse)
    DRE_OPT_I("gemm_swizzle", gemm_swizzle)
    DRE_OPT_I("mf_swizzle", mf_swizzle)
    DRE_OPT_I("ros2_tight", ros2_tight)
    DRE_OPT_D("compress_sketch_ratio", compress_sketch_ratio)
    DRE_OPT_I("top_inverse_max_rows", top_inverse_max_rows)
    DRE_OPT_I("mf_subtree", mf_subtree)
    DRE_OPT_I("setup_streams", setup_streams)
    DRE_OPT_I("x_side_stream", x_side_stream)
    DRE_OPT_I("side_after_panels", side_after_panels)
    DRE_OPT_I("setup_batched", setup_batched)
    DRE_OPT_I("dense_warm", dense_warm)
    DRE_OPT_I("dense_gj_panel", dense_gj_panel)
    DRE_OPT_I("sym_eig_method", sym_eig_method)
    DRE_OPT_I("side_prefetch", side_prefetch)
    DRE_OPT_I("side_gate", side_gate)
    DRE_OPT_I("recurrence_wide", recurrence_wide)
    DRE_OPT_I("xwarm_sx", xwarm_sx)
    DRE_OPT_I("prefetch_batch", prefetch_batch)
    DRE_OPT_I("dense_x_max_n", dense_x_max_n)
    DRE_OPT_I("dense_x_max_k", dense_x_max_k)
    DRE_OPT_I("final_x_lazy", final_x_lazy)
    DRE_OPT_I("adi_group", adi_group)
    DRE_OPT_I("adi_group_max_n", adi_group_max_n)
    DRE_OPT_I("adi_fan", adi_fan)
    DRE_OPT_I("ros1_recurrence", ros1_recurrence)
    DRE_OPT_D("adi_fan_max_coef", adi_fan_max_coef)
    DRE_OPT_I("shard_min_cols", shard_min_cols)
    DRE_OPT_I("comm_host_async", comm_host_async)
    DRE_OPT_I("x_compress_every", x_compress_every)
    DRE_OPT_D("pivot_growth_warn", pivot_growth_warn)
    DRE_OPT_D("pivot_growth_fail", pivot_growth_fail)
    DRE_OPT_D("pivot_static", pivot_static)
    DRE_OPT_I("pivot_refine_steps", pivot_refine_steps)
#undef DRE_OPT_I
#undef DRE_OPT_D
    return r;
}
int dre_ctx_set_option(dre_ctx* ctx, const char* name, double value) {
    return guarded(ctx, [&] {
        const std::string key = name ? name : "";
        if (!(value == value)) throw Error(ERR_INVALID, "dre_ctx_set_option: the value of '" + key + "' is not a number");
        if (key == "shard_emulate") {
            // ONE process plays `value` ranks of the column-sharded ADI step one after the other (tests of the blocking logic on one GPU)
            if (!ctx->c.comm) ctx->c.comm = std::make_shared<Comm>();
            ctx->c.comm->emulate = (int)value;
            return;
        }
        if (key == "dense_gj_panel" && !(value == 0.0 || value == 1.0 || value == 2.0))
            throw Error(ERR_INVALID, "dre_ctx_set_option: dense_gj_panel must be 0 (auto), 1 (register) or 2 (tournament)");
        if (key == "sym_eig_method" && !(value == 0.0 || value == 1.0))
            throw Error(ERR_INVALID, "dre_ctx_set_option: sym_eig_method must be 0 (Householder + QL) or 1 (block Jacobi)");
        const OptionRef r = option_ref(ctx->c, key);
        if (r.i) *r.i = (int)value;
        else if (r.d) *r.d = value;
        else throw Error(ERR_INVALID, "dre_ctx_set_option: unknown option '" + key + "'");
    });
}
int dre_ctx_get_option(dre_ctx* ctx, const char* name, double* value) {
    return guarded(ctx, [&] {
        const std::string key = name ? name : "";
        if (!value) throw Error(ERR_INVALID, "dre_ctx_get_option: null output");
        if (key == "shard_emulate") { *value = ctx->c.comm ? (double)ctx->c.comm->emulate : 0.0; return; }
        const OptionRef r = option_ref(ctx->c, key);
        if (r.i) *value = (double)*r.i;
        else if (r.d) *value = *r.d;
        else throw Error(ERR_INVALID, "dre_ctx_get_option: unknown option '" + key + "'");
    });
}
// Both contexts of a library context are timed (the side context carries the work that runs beside the main stream): enable/reset act on
// both, count/get see the per-class sums.
// every context that carries work of this library context: main, side, and the helper contexts of both
static void for_each_timed(dre_ctx* ctx, const std::function<void(Ctx&)>& f) {
    auto visit = [&](Ctx& c) { f(c); for (auto& h : c.helpers) if (h && h->timer) f(*h); };
    visit(ctx->c);
    if (ctx->c.side && ctx->c.side->timer) visit(*ctx->c.side);
}
static void prof_collect_merge(dre_ctx* ctx) {
    ctx->merged.clear();
    for_each_timed(ctx, [&](Ctx& c) {
        c.timer->collect(&c);
        for (auto& kv : c.timer->stats) {
            auto& d = ctx->merged[kv.first];
            d.ms += kv.second.ms; d.launches += kv.second.launches; d.bytes += kv.second.bytes; d.flops += kv.second.flops;
        }
    });
}
int dre_prof_enable(dre_ctx* ctx, int on) {
    return guarded(ctx, [&] {
        ctx->c.prof_side = on != 0;
        for_each_timed(ctx, [&](Ctx& c) { c.timer->collect(&c); c.timer->enabled = on != 0; });
    });
}
int dre_prof_reset(dre_ctx* ctx) {
    return guarded(ctx, [&] {
        for_each_timed(ctx, [&](Ctx& c) { c.timer->collect(&c); c.timer->stats.clear(); });
        ctx->merged.clear();
    });
}
int dre_prof_count(dre_ctx* ctx, int* n) {
    return guarded(ctx, [&] { prof_collect_merge(ctx); *n = (int)ctx->merged.size(); });
}
int dre_prof_get(dre_ctx* ctx, int i, char* name, int name_len, double* ms, int64_t* launches, double* bytes, double* flops) {
    return guarded(ctx, [&] {
        auto& st = ctx->merged;
        DRE_REQUIRE(i >= 0 && i < (int)st.size(), "dre_prof_get: index out of range");
        auto it = st.begin();
        std::advance(it, i);
        std::snprintf(name, name_len, "%s", it->first.c_str());
        *ms = it->second.ms; *launches = it->second.launches; *bytes = it->second.bytes; *flops = it->second.flops;
    });
}

// ---- dense -------------------------------------------------------------------------------------
int dre_dense_upload(dre_ctx* ctx, int rows, int cols, const double* host, int ld, dre_dense** out) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(rows >= 0 && cols >= 0 && ld >= std::max(rows, 1), "dre_dense_upload: bad shape");
        auto* d = new dre_dense();
        d->m = Mat(&ctx->c, rows, cols);
        if (rows > 0 && cols > 0) {
            DRE_HIP(hipMemcpy2DAsync(d->m.p, (size_t)d->m.ld * sizeof(double), host, (size_t)ld * sizeof(double),
                                     (size_t)rows * sizeof(double), cols, hipMemcpyHostToDevice, ctx->c.stream));
            DRE_HIP(hipStreamSynchronize(ctx->c.stream));
        }
        *out = d;
    });
}
int dre_dense_create(dre_ctx* ctx, int rows, int cols, dre_dense** out) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(rows >= 0 && cols >= 0, "dre_dense_create: bad shape");
        auto* d = new dre_dense();
        d->m = Mat(&ctx->c, rows, cols);
        fill_mat(&ctx->c, d->m, 0.0);
        *out = d;
    });
}
static void download_mat(Ctx* c, const Mat& m, double* host, int ld) {
    DRE_REQUIRE(ld >= std::max(m.rows, 1), "download: leading dimension too small");
    if (m.rows > 0 && m.cols > 0) {
        DRE_HIP(hipMemcpy2DAsync(host, (size_t)ld * sizeof(double), m.p, (size_t)m.ld * sizeof(double),
                                 (size_t)m.rows * sizeof(double), m.cols, hipMemcpyDeviceToHost, c->stream));
    }
    DRE_HIP(hipStreamSynchronize(c->stream));
}
int dre_dense_download(dre_ctx* ctx, const dre_dense* a, double* host, int ld) {
    return guarded(ctx, [&] { download_mat(&ctx->c, a->m, host, ld); });
}
// device-to-device interop with buffers the caller owns (e.g. the exchange tensors handed to RCCL): column-major, leading dimension ld
int dre_dense_from_device(dre_ctx* ctx, int rows, int cols, const double* src_dev, int ld, dre_dense** out) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(rows >= 0 && cols >= 0 && ld >= std::max(rows, 1), "dre_dense_from_device: bad shape");
        auto* d = new dre_dense();
        d->m = Mat(&ctx->c, rows, cols);
        if (rows > 0 && cols > 0)
            DRE_HIP(hipMemcpy2DAsync(d->m.p, (size_t)d->m.ld * sizeof(double), src_dev, (size_t)ld * sizeof(double), (size_t)rows * sizeof(double), cols,
                                     hipMemcpyDeviceToDevice, ctx->c.stream));
        DRE_HIP(hipStreamSynchronize(ctx->c.stream));
        *out = d;
    });
}
int dre_dense_to_device(dre_ctx* ctx, const dre_dense* a, double* dst_dev, int ld) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(ld >= std::max(a->m.rows, 1), "dre_dense_to_device: bad leading dimension");
        if (a->m.rows > 0 && a->m.cols > 0)
            DRE_HIP(hipMemcpy2DAsync(dst_dev, (size_t)ld * sizeof(double), a->m.p, (size_t)a->m.ld * sizeof(double), (size_t)a->m.rows * sizeof(double), a->m.cols,
                                     hipMemcpyDeviceToDevice, ctx->c.stream));
        DRE_HIP(hipStreamSynchronize(ctx->c.stream));
    });
}
int dre_dense_shape(const dre_dense* a, int* rows, int* cols) { *rows = a->m.rows; *cols = a->m.cols; return DRE_OK; }
int dre_dense_free(dre_ctx*, dre_dense* a) { delete a; return DRE_OK; }

// ---- pencil ------------------------------------------------------------------------------------
static int pencil_create_impl(dre_ctx* ctx, bool upload, int n, const int64_t* Ep, const int64_t* Ei, const double* Ev,
                              const int64_t* Ap, const int64_t* Ai, const double* Av, int base, int leaf, dre_pencil** out) {
    return guarded(ctx, [&] {
        auto* h = new dre_pencil();
        try {
            h->p = pencil_create(ctx ? &ctx->c : nullptr, n, Ep, Ei, Ev, Ap, Ai, Av, base, leaf, upload, &h->hE, &h->hA);
        } catch (...) { delete h; throw; }
        *out = h;
    });
}
int dre_pencil_create(dre_ctx* ctx, int n, const int64_t* Ep, const int64_t* Ei, const double* Ev, const int64_t* Ap,
                      const int64_t* Ai, const double* Av, int base, int leaf, dre_pencil** out) {
    return pencil_create_impl(ctx, true, n, Ep, Ei, Ev, Ap, Ai, Av, base, leaf, out);
}
int dre_pencil_create_host(int n, const int64_t* Ep, const int64_t* Ei, const double* Ev, const int64_t* Ap,
                           const int64_t* Ai, const double* Av, int base, int leaf, dre_pencil** out) {
    return pencil_create_impl(nullptr, false, n, Ep, Ei, Ev, Ap, Ai, Av, base, leaf, out);
}
int dre_pencil_free(dre_pencil* p) { delete p; return DRE_OK; }
int dre_pencil_info(const dre_pencil* p, int64_t* info) {
    const Symbolic& S = p->p->sym;
    info[0] = S.n; info[1] = (int64_t)S.idx.size(); info[2] = S.nnodes; info[3] = S.nlevels; info[4] = S.max_front;
    info[5] = S.max_sep; info[6] = S.factor_nnz; info[7] = S.fronts_size;
    return DRE_OK;
}
int dre_pencil_get_array(const dre_pencil* p, const char* name, int64_t* out, int64_t cap, int64_t* len) {
    const Symbolic& S = p->p->sym;
    std::string nm(name);
    auto put_i = [&](const std::vector<int>& v) { *len = (int64_t)v.size(); if (out) for (int64_t i = 0; i < std::min<int64_t>(cap, v.size()); ++i) out[i] = v[i]; return DRE_OK; };
    auto put_l = [&](const std::vector<int64_t>& v) { *len = (int64_t)v.size(); if (out) for (int64_t i = 0; i < std::min<int64_t>(cap, v.size()); ++i) out[i] = v[i]; return DRE_OK; };
    if (nm == "perm") return put_i(S.perm);
    if (nm == "iperm") return put_i(S.iperm);
    if (nm == "ptr") return put_i(S.ptr);
    if (nm == "idx") return put_i(S.idx);
    if (nm == "first") return put_i(S.first);
    if (nm == "size") return put_i(S.size);
    if (nm == "parent") return put_i(S.parent);
    if (nm == "level") return put_i(S.level);
    if (nm == "child_ptr") return put_i(S.child_ptr);
    if (nm == "child_idx") return put_i(S.child_idx);
    if (nm == "bptr") return put_i(S.bptr);
    if (nm == "bidx") return put_i(S.bidx);
    if (nm == "cmap_ptr") return put_i(S.cmap_ptr);
    if (nm == "cmap") return put_i(S.cmap);
    if (nm == "lvl_ptr") return put_i(S.lvl_ptr);
    if (nm == "lvl_nodes") return put_i(S.lvl_nodes);
    if (nm == "front_off") return put_l(S.front_off);
    if (nm == "inv_off") return put_l(S.inv_off);
    if (nm == "upd_off") return put_l(S.upd_off);
    if (nm == "asm_dest") return put_l(S.asm_dest);
    return DRE_ERR_INVALID;
}
int dre_pencil_get_values(const dre_pencil* p, int which, double* out, int64_t cap) {
    const std::vector<double>& v = which == 0 ? p->hE : p->hA;
    if ((int64_t)v.size() > cap) return DRE_ERR_INVALID;
    std::memcpy(out, v.data(), v.size() * sizeof(double));
    return DRE_OK;
}

// helpers: rows of user-ordered matrices <-> solver ordering
static Mat to_solver_order(Ctx* c, const dre_pencil* pen, const Mat& src) {
    if (!pen) return src;
    DRE_REQUIRE(src.rows == pen->p->n, "matrix row count does not match the pencil");
    Mat dst(c, src.rows, src.cols);
    permute_rows(c, src, pen->p->perm.p, dst);     // dst(new,:) = src(perm[new],:)
    return dst;
}
static Mat to_user_order(Ctx* c, const dre_pencil* pen, const Mat& src) {
    if (!pen) return src;
    Mat dst(c, src.rows, src.cols);
    permute_rows(c, src, pen->p->iperm.p, dst);    // dst(old,:) = src(iperm[old],:)
    return dst;
}

// ---- kernels -----------------------------------------------------------------------------------
int dre_gemm(dre_ctx* ctx, int tA, int tB, double alpha, const dre_dense* A, const dre_dense* B, double beta, dre_dense* C) {
    return guarded(ctx, [&] { gemm(&ctx->c, tA != 0, tB != 0, alpha, A->m, B->m, beta, C->m); });
}
// ---- dre_gemm_probe: the internal GEMM entry points one by one (test and diagnostic surface) ------------------------------------------
namespace {
int64_t probe_cap(const dre_dense* d) {          // elements of the buffer from the matrix's first element on
    if (!d || !d->m.buf || !d->m.p) return -1;
    const char* base = (const char*)d->m.buf->p;
    const char* p = (const char*)d->m.p;
    if (p < base || (size_t)(p - base) > d->m.buf->bytes) return -1;
    return (int64_t)((d->m.buf->bytes - (size_t)(p - base)) / sizeof(double));
}
void probe_check(const dre_gemm_view* v, const char* what, int64_t count = 1, int64_t stride = 0) {
    DRE_REQUIRE(v && v->buf, std::string("dre_gemm_probe: missing view ") + what);
    DRE_REQUIRE(probe_view_fits(probe_cap(v->buf), v->offset, v->ld, v->rows, v->cols, count, stride),
                std::string("dre_gemm_probe: view ") + what + " does not lie inside its buffer");
}
double* probe_ptr(const dre_gemm_view* v) { return v->buf->m.p + v->offset; }
void probe_mat(const dre_gemm_view* v, Mat& m) { m.buf = v->buf->m.buf; m.p = probe_ptr(v); m.rows = v->rows; m.cols = v->cols; m.ld = v->ld; }
}  // namespace

int dre_gemm_probe(dre_ctx* ctx, int kind, int transA, int transB, double alpha, const dre_gemm_view* A, const dre_gemm_view* B, double beta,
                   const dre_gemm_view* C, const dre_gemm_probe_options* opt, int* splits_out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const dre_gemm_probe_options none = {};
        const dre_gemm_probe_options& o = opt ? *opt : none;
        const bool tA = transA != 0, tB = transB != 0;
        DRE_REQUIRE(kind >= DRE_PROBE_GEMM && kind <= DRE_PROBE_GEMM_SYM, "dre_gemm_probe: unknown kind");
        const int batch = o.batch > 0 ? o.batch : 1;
        DRE_REQUIRE(o.batch >= 0 && batch <= 65535, "dre_gemm_probe: batch");
        const bool stacked = kind == DRE_PROBE_GEMM_STRIDED || kind == DRE_PROBE_GEMM_Z;
        // what each kind can take
        const bool takes_done = kind == DRE_PROBE_GEMM || kind == DRE_PROBE_GEMM_THIN || kind == DRE_PROBE_GEMM_ROWS || kind == DRE_PROBE_GEMM_Z;
        const bool takes_count = kind == DRE_PROBE_GEMM_BATCHED || kind == DRE_PROBE_GEMM_ROWS || kind == DRE_PROBE_GEMM_SYM;
        DRE_REQUIRE(!o.use_done || takes_done, "dre_gemm_probe: this kind takes no done flag");
        DRE_REQUIRE(!o.use_count || takes_count, "dre_gemm_probe: this kind takes no device-side count");
        DRE_REQUIRE(!o.tile_sumsq || kind == DRE_PROBE_GEMM, "dre_gemm_probe: tile_sumsq belongs to gemm");
        DRE_REQUIRE((!o.member_on && !o.coef) || kind == DRE_PROBE_GEMM_STRIDED, "dre_gemm_probe: member_on and coef belong to gemm_strided");
        DRE_REQUIRE(!o.rowmap || kind == DRE_PROBE_GEMM_ROWS || kind == DRE_PROBE_GEMM_Z, "dre_gemm_probe: rowmap belongs to the reduce kinds");
        DRE_REQUIRE(stacked || o.batch <= 1, "dre_gemm_probe: this kind takes no batch");
        DRE_REQUIRE((o.nprod == 0 && !o.prod) || kind == DRE_PROBE_GEMM_BATCHED, "dre_gemm_probe: products belong to gemm_batched");
        DRE_REQUIRE(!o.use_count || (o.per >= 1 && o.nmax >= 0), "dre_gemm_probe: count needs per >= 1, nmax >= 0");

        int M = 0, N = 0, K = 0;
        if (kind != DRE_PROBE_GEMM_BATCHED) {
            const int64_t sa = stacked ? o.stride_a : 0, sb = stacked ? o.stride_b : 0;
            const int64_t sc = kind == DRE_PROBE_GEMM_STRIDED ? o.stride_c : (kind == DRE_PROBE_GEMM_Z ? o.cz : 0);
            probe_check(A, "A", batch, sa);
            probe_check(B, "B", batch, sb);
            probe_check(C, "C", batch, sc);
            if (kind == DRE_PROBE_GEMM_SYM) {
                M = N = C->rows; K = A->cols;
                DRE_REQUIRE(C->cols == M && A->rows == M && B->rows == M && B->cols == K && !tA && !tB, "dre_gemm_probe: gemm_sym_update takes A, B of n x K and C of n x n");
            } else {
                M = tA ? A->cols : A->rows; K = tA ? A->rows : A->cols; N = tB ? B->rows : B->cols;
                DRE_REQUIRE((tB ? B->cols : B->rows) == K, "dre_gemm_probe: inner dimensions differ");
                DRE_REQUIRE(C->cols == N, "dre_gemm_probe: C has the wrong number of columns");
                const bool mapped = kind == DRE_PROBE_GEMM_ROWS || (kind == DRE_PROBE_GEMM_Z && o.rowmap);
                DRE_REQUIRE(mapped ? C->rows >= M : C->rows == M, "dre_gemm_probe: C has the wrong number of rows");
                DRE_REQUIRE(kind != DRE_PROBE_GEMM_ROWS || o.rowmap, "dre_gemm_probe: gemm_reduce_rows needs a rowmap");
                DRE_REQUIRE(kind != DRE_PROBE_GEMM_THIN || !tB, "dre_gemm_probe: gemm_thin has no transposed B");
            }
            if (o.rowmap) for (int i = 0; i < M; ++i) DRE_REQUIRE(o.rowmap[i] >= 0 && o.rowmap[i] < C->rows, "dre_gemm_probe: rowmap entry outside C");
        }

        // device-side control blocks
        DevArr<AdiState> st;
        const AdiState* stp = nullptr;
        if (o.use_done || o.use_count) {
            std::vector<AdiState> h(1);
            std::memset(h.data(), 0, sizeof(AdiState));
            h[0].done = o.use_done ? o.done : 0; h[0].iters = o.iters;
            st = DevArr<AdiState>(c, 1); st.upload(c, h);
            stp = st.p;
        }
        const AdiState* done_st = o.use_done ? stp : nullptr;
        DevCount dc;
        if (o.use_count) { dc.st = stp; dc.base = o.base; dc.nmax = o.nmax; dc.per = o.per; }
        DevArr<int> rowmap;
        if (o.rowmap && M > 0) { rowmap = DevArr<int>(c, (size_t)M); rowmap.upload(c, o.rowmap, (size_t)M); }
        int splits = 1;

        switch (kind) {
        case DRE_PROBE_GEMM: {
            double* ss = nullptr;
            if (o.tile_sumsq) {
                DRE_REQUIRE(probe_cap(o.tile_sumsq) >= (int64_t)gemm_num_tiles(M, N), "dre_gemm_probe: tile_sumsq is too small");
                ss = o.tile_sumsq->m.p;
            }
            if (M > 0 && N > 0 && !(ss && K > 64)) splits = gemm_split_plan(c, ceil_div(M, 64) * ceil_div(N, 64), K);
            gemm(c, tA, tB, M, N, K, alpha, probe_ptr(A), A->ld, probe_ptr(B), B->ld, beta, probe_ptr(C), C->ld, done_st, "gemm_probe", ss);
            break;
        }
        case DRE_PROBE_GEMM_THIN:
            gemm_thin(c, tA, M, N, K, alpha, probe_ptr(A), A->ld, probe_ptr(B), B->ld, beta, probe_ptr(C), C->ld, done_st, "gemm_probe");
            break;
        case DRE_PROBE_GEMM_STRIDED: {
            DevArr<BatchCtl> ctl;
            BatchMask mask;
            if (o.member_on) {
                std::vector<BatchCtl> h((size_t)batch);
                std::memset(h.data(), 0, h.size() * sizeof(BatchCtl));
                for (int b = 0; b < batch; ++b) h[(size_t)b].fail = o.member_on[b] ? 0 : DRE_ERR_SINGULAR;
                ctl = DevArr<BatchCtl>(c, (size_t)batch); ctl.upload(c, h);
                mask.ctl = ctl.p;
            }
            DevArr<double> coef;
            if (o.coef) {
                DRE_REQUIRE(o.coef_stride >= 2 && o.coef_stride <= 4096, "dre_gemm_probe: coef_stride");
                coef = DevArr<double>(c, (size_t)batch * (size_t)o.coef_stride);
                coef.upload(c, o.coef, (size_t)batch * (size_t)o.coef_stride);
            }
            gemm_strided(c, batch, tA, tB, M, N, K, alpha, probe_ptr(A), A->ld, (size_t)o.stride_a, probe_ptr(B), B->ld, (size_t)o.stride_b, beta, probe_ptr(C),
                         C->ld, (size_t)o.stride_c, mask, "gemm_probe", o.coef ? coef.p : nullptr, o.coef ? (size_t)o.coef_stride : 0);
            c->sync();          // (the uploaded blocks live until here)
            break;
        }
        case DRE_PROBE_GEMM_BATCHED: {
            DRE_REQUIRE(o.nprod >= 0 && o.nprod <= 65535 && (o.nprod == 0 || o.prod), "dre_gemm_probe: product list");
            std::vector<GemmBatchDesc> descs;
            for (int i = 0; i < o.nprod; ++i) {
                const dre_gemm_product& p = o.prod[i];
                probe_check(&p.A, "A of a product"); probe_check(&p.B, "B of a product"); probe_check(&p.C, "C of a product");
                DRE_REQUIRE(p.A.cols == p.B.rows && p.C.rows == p.A.rows && p.C.cols == p.B.cols, "dre_gemm_probe: shapes of a product");
                GemmBatchDesc d;
                d.A = probe_ptr(&p.A); d.B = probe_ptr(&p.B); d.C = probe_ptr(&p.C); d.copy_dst = nullptr; d.alpha = p.alpha;
                d.M = p.A.rows; d.N = p.B.cols; d.K = p.A.cols; d.lda = p.A.ld; d.ldb = p.B.ld; d.ldc = p.C.ld; d.ldcopy = 0;
                if (p.copy_dst.buf) {
                    probe_check(&p.copy_dst, "copy_dst of a product");
                    DRE_REQUIRE(p.copy_dst.rows == d.M && p.copy_dst.cols == d.K, "dre_gemm_probe: copy_dst has the shape of A");
                    d.copy_dst = probe_ptr(&p.copy_dst); d.ldcopy = p.copy_dst.ld;
                }
                descs.push_back(d);
            }
            gemm_batched(c, descs, "gemm_probe", dc);
            break;
        }
        case DRE_PROBE_GEMM_ROWS: {
            BufP pb = gemm_partials(c, tA, tB, M, N, K, probe_ptr(A), A->ld, probe_ptr(B), B->ld, &splits, done_st, "gemm_probe", dc);
            gemm_reduce_rows(c, M, N, splits, (const double*)pb->p, rowmap.p, probe_ptr(C), C->ld, done_st);
            break;
        }
        case DRE_PROBE_GEMM_Z: {
            GemmZ zb;
            for (int z = 0; z < MF_ZMAX; ++z) {       // (a batch beyond MF_ZMAX is for gemm_partials_z to refuse)
                const int zz = std::min(z, batch - 1);
                zb.A[z] = probe_ptr(A) + (size_t)zz * (size_t)o.stride_a; zb.B[z] = probe_ptr(B) + (size_t)zz * (size_t)o.stride_b;
            }
            BufP pb = gemm_partials_z(c, tA, tB, M, N, K, zb, batch, A->ld, B->ld, &splits, done_st, "gemm_probe");
            gemm_reduce_z(c, M, N, splits, batch, (const double*)pb->p, o.rowmap ? rowmap.p : nullptr, probe_ptr(C), C->ld, (long)o.cz, done_st);
            break;
        }
        case DRE_PROBE_GEMM_SYM: {
            Mat Am, Bm, Xm;
            probe_mat(A, Am); probe_mat(B, Bm); probe_mat(C, Xm);
            if (M > 0 && K > 0) splits = gemm_split_plan(c, ceil_div(M, 64) * ceil_div(M, 64), K);
            gemm_sym_update(c, Am, Bm, Xm, "gemm_probe", dc);
            break;
        }
        }
        c->sync();
        if (splits_out) *splits_out = splits;
    });
}
int dre_spmm(dre_ctx* ctx, const dre_pencil* p, int which, double alpha, const dre_dense* X, double beta, dre_dense* Y) {
    return guarded(ctx, [&] {
        const Pencil& P = *p->p;
        DRE_REQUIRE(P.has_device, "pencil was created host-only");
        Mat Xs = to_solver_order(&ctx->c, p, X->m);
        Mat Ys = to_solver_order(&ctx->c, p, Y->m);
        spmm(&ctx->c, P, which == 0 ? P.valEt.p : P.valAt.p, Xs, Ys, alpha, beta);
        Mat Yu = to_user_order(&ctx->c, p, Ys);
        copy_mat(&ctx->c, Yu, Y->m);
    });
}
int dre_ctx_set_orthf(dre_ctx* ctx, dre_orthf_fn fn, void* user) {
    return guarded(ctx, [&] { ctx->c.orthf_fn = fn; ctx->c.orthf_user = user; if (ctx->c.side) { ctx->c.side->orthf_fn = fn; ctx->c.side->orthf_user = user; } });
}
int dre_orthf(dre_ctx* ctx, const dre_dense* L, dre_dense** Qo, dre_dense** Ro) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        Mat A(c, L->m.rows, L->m.cols);
        copy_mat(c, L->m, A);
        QRFact f = qr_factor(c, A);
        auto* Q = new dre_dense();
        Q->m = Mat(c, f.m, f.kq);
        set_identity(c, Q->m, 1.0);
        qr_apply_q(c, f, Q->m, false);
        auto* R = new dre_dense();
        R->m = f.R;
        *Qo = Q; *Ro = R;
    });
}
int dre_sym_eig(dre_ctx* ctx, const dre_dense* S, double tolfac, dre_dense** values, dre_dense** vectors) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        Mat A(c, S->m.rows, S->m.cols);
        copy_mat(c, S->m, A);
        // (this entry IS the Householder + QL solver, whatever sym_eig_method says; the Jacobi solver has dre_sym_eig_jacobi)
        struct Method0 { Ctx* c; int was; ~Method0() { c->sym_eig_method = was; } } method0{c, c->sym_eig_method};
        c->sym_eig_method = 0;
        SymEig e = sym_eig(c, A, tolfac > 0 ? tolfac : 4.0);
        std::vector<int> ids(e.j);
        for (int i = 0; i < e.j; ++i) ids[i] = i;
        std::sort(ids.begin(), ids.end(), [&](int a, int b) { return e.w[a] < e.w[b]; });
        std::vector<double> w(e.j);
        for (int i = 0; i < e.j; ++i) w[i] = e.w[ids[i]];
        auto* V = new dre_dense();
        V->m = sym_eig_backtransform(c, e, ids);
        auto* W = new dre_dense();
        W->m = Mat(c, e.j, 1);
        if (e.j) {
            DRE_HIP(hipMemcpyAsync(W->m.p, w.data(), e.j * sizeof(double), hipMemcpyHostToDevice, c->stream));
            DRE_HIP(hipStreamSynchronize(c->stream));
        }
        *values = W; *vectors = V;
    });
}
// ---- dre_sym_eig_probe: the stages of the Householder + QL solver one by one (test and diagnostic surface) --------------------------------
int dre_sym_eig_probe(dre_ctx* ctx, const dre_dense* S, double tolfac, int want_eig, double abs_tol, int floor_mode, double deflate, const int32_t* ids,
                      int nids, int64_t* ii, double* snorm, dre_dense** d, dre_dense** e, dre_dense** tau, dre_dense** V, dre_dense** w, dre_dense** Z,
                      dre_dense** B) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        dre_dense** outs[7] = {d, e, tau, V, w, Z, B};
        for (dre_dense** o : outs) if (o) *o = nullptr;
        DRE_REQUIRE(S && ii, "dre_sym_eig_probe: null argument");
        DRE_REQUIRE(S->m.rows == S->m.cols, "dre_sym_eig_probe: square matrix expected");
        DRE_REQUIRE(S->m.rows <= 8192, "dre_sym_eig_probe: order above 8192 not supported by the single-workgroup reduction");
        DRE_REQUIRE(nids <= 0 || ids, "dre_sym_eig_probe: ids missing");
        DRE_REQUIRE(nids == 0 || B, "dre_sym_eig_probe: ids without a place for B");
        DRE_REQUIRE(tolfac > 0.0 && deflate >= 0.0, "dre_sym_eig_probe: tolfac must be positive, deflate not negative");
        const int q = S->m.rows;
        Mat A(c, q, q);
        copy_mat(c, S->m, A);
        struct Method0 { Ctx* c; int was; ~Method0() { c->sym_eig_method = was; } } method0{c, c->sym_eig_method};
        c->sym_eig_method = 0;
        SymEig r = sym_eig(c, A, tolfac, want_eig != 0, abs_tol, floor_mode != 0, deflate);
        std::vector<int> cols;
        if (nids < 0) { cols.resize((size_t)r.j); for (int i = 0; i < r.j; ++i) cols[(size_t)i] = i; }          // (every column)
        else cols.assign(ids, ids + nids);
        for (int id : cols) DRE_REQUIRE(id >= 0 && id < r.j, "dre_sym_eig_probe: an entry of ids lies outside [0, jdim)");
        ii[0] = r.j; ii[1] = r.nref; ii[2] = q;
        if (snorm) *snorm = r.snorm;
        std::vector<std::unique_ptr<dre_dense>> made;          // (an error below frees what was made; the handles go out together at the end)
        auto column = [&](const double* src, bool on_host, int n) {
            made.emplace_back(new dre_dense());
            made.back()->m = Mat(c, n, 1);
            if (n) DRE_HIP(hipMemcpyAsync(made.back()->m.p, src, (size_t)n * sizeof(double), on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
            return made.back().get();
        };
        auto matrix = [&](const Mat& M) { made.emplace_back(new dre_dense()); made.back()->m = M; return made.back().get(); };
        const bool has_z = want_eig && r.j > 0;
        dre_dense* od = d ? column(r.d.p, false, r.j) : nullptr;
        dre_dense* oe = e ? column(r.e.p, false, std::max(r.j - 1, 0)) : nullptr;
        dre_dense* ot = tau ? column(r.tau.p, false, q) : nullptr;
        dre_dense* oV = V ? matrix(q ? r.V : Mat(c, 0, 0)) : nullptr;
        dre_dense* ow = (w && has_z) ? column(r.w.data(), true, r.j) : nullptr;
        dre_dense* oZ = (Z && has_z) ? matrix(r.Z) : nullptr;
        dre_dense* oB = nullptr;
        if (B && !cols.empty()) oB = matrix(sym_eig_backtransform(c, r, cols));
        c->sync();          // (r.w is host memory of this scope)
        dre_dense* res[7] = {od, oe, ot, oV, ow, oZ, oB};
        for (int k = 0; k < 7; ++k) if (outs[k]) *outs[k] = res[k];
        for (auto& m : made) m.release();
    });
}
// ---- dre_warm_probe: the kernels of the warm-started compression (warm.hip) on caller-supplied operands (test and diagnostic surface) -------
// Every launch goes through warm_project, warm_z, warm_zapply, warm_small, warm_eig, warm_finish or warm_chain_jacobi, with the buffer shapes of
// their callers (dense_x.hip, compress_warm; ldlt.hip, warm_compress_eig).
int dre_warm_probe(dre_ctx* ctx, const dre_warm_probe_args* args) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(args, "dre_warm_probe: null argument");
        const dre_warm_probe_args& p = *args;
        const int st = p.stage, n = p.n, q = p.q, m = p.m, kl = p.kl, qn = p.qn;
        DRE_REQUIRE(st >= DRE_WARM_PROBE_PROJECT && st <= DRE_WARM_PROBE_CHAIN, "dre_warm_probe: unknown stage");
        DRE_REQUIRE(p.ldpad >= 0 && p.ldpad <= 64, "dre_warm_probe: ldpad must lie in 0 .. 64");
        const bool rows_n = st != DRE_WARM_PROBE_SMALL && st != DRE_WARM_PROBE_EIG;
        if (rows_n) DRE_REQUIRE(n >= 1 && n <= 65536, "dre_warm_probe: n must lie in 1 .. 65536");
        if (st == DRE_WARM_PROBE_PROJECT || st == DRE_WARM_PROBE_Z || st == DRE_WARM_PROBE_ZAPPLY || st == DRE_WARM_PROBE_SMALL || st == DRE_WARM_PROBE_CHAIN)
            DRE_REQUIRE(q >= 1 && q <= 64, "dre_warm_probe: q must lie in 1 .. 64");
        if (st == DRE_WARM_PROBE_Z || st == DRE_WARM_PROBE_CHAIN) DRE_REQUIRE(n <= 1024, "dre_warm_probe: n above 1024 (warm_z keeps all of Z in LDS)");
        if (st == DRE_WARM_PROBE_PROJECT) DRE_REQUIRE(p.Q && p.Yf && p.Pf, "dre_warm_probe: Q, Yf or Pf missing");
        if (st == DRE_WARM_PROBE_Z) DRE_REQUIRE(p.Z1 && p.Cw && p.Res, "dre_warm_probe: Z1, Cw or Res missing");
        if (st == DRE_WARM_PROBE_ZAPPLY) DRE_REQUIRE(p.Z1 && p.Cw, "dre_warm_probe: Z1 or Cw missing");
        if (st == DRE_WARM_PROBE_SMALL || st == DRE_WARM_PROBE_CHAIN) {
            const int mm = st == DRE_WARM_PROBE_CHAIN ? q + 16 : m;
            DRE_REQUIRE(mm == q || mm == q + 16, "dre_warm_probe: m must be q or q + 16");
            DRE_REQUIRE(mm <= 80, "dre_warm_probe: m above 80");
            DRE_REQUIRE(qn >= 1 && qn <= mm && (st != DRE_WARM_PROBE_CHAIN || qn <= 64), "dre_warm_probe: qn must lie in 1 .. m (chain: at most 64)");
            DRE_REQUIRE(kl >= 1 && kl <= qn, "dre_warm_probe: kl must lie in 1 .. qn");
            DRE_REQUIRE(p.nparts >= 0 && p.nparts <= (1 << 24) && (p.nparts == 0 || p.parts), "dre_warm_probe: nparts without parts");
            DRE_REQUIRE(p.budget_frac >= 0.0 && p.budget_frac <= 1.0, "dre_warm_probe: budget_frac must lie in 0 .. 1");
        }
        if (st == DRE_WARM_PROBE_SMALL) {
            DRE_REQUIRE(p.mode == 0 || p.mode == 1, "dre_warm_probe: mode must be 0 or 1");
            DRE_REQUIRE(p.Cc, "dre_warm_probe: Cc missing");
        }
        if (st == DRE_WARM_PROBE_EIG) {
            DRE_REQUIRE(m >= 1 && m <= 80, "dre_warm_probe: m must lie in 1 .. 80");
            DRE_REQUIRE(p.S, "dre_warm_probe: S missing");
        }
        if (st == DRE_WARM_PROBE_FINISH) {
            DRE_REQUIRE(q >= 1 && q <= 80, "dre_warm_probe: q must lie in 1 .. 80");
            DRE_REQUIRE(kl >= 1 && kl <= 80, "dre_warm_probe: kl must lie in 1 .. 80");
            DRE_REQUIRE(p.Q && p.Wk && p.Yp && p.Pp && p.tols_in, "dre_warm_probe: B, Wk, Yp, Pp or tols_in missing");
        }
        if (st == DRE_WARM_PROBE_CHAIN) DRE_REQUIRE(p.Res && p.basis, "dre_warm_probe: Res or basis missing");
        // (the arguments are judged without a context, so that the refusals can be tested on a machine without a device)
        DRE_REQUIRE(ctx, "dre_warm_probe: arguments accepted, context missing");
        Ctx* c = &ctx->c;
        const int ldn = n + p.ldpad;
        // a matrix of `rows` rows prefilled with NaN (all bits set): the view has the rows the entry points expect, the allocation ld of them
        auto nan_mat = [&](int rows, int ld, int cols) {
            Mat full(c, ld, cols);
            DRE_HIP(hipMemsetAsync(full.p, 0xFF, (size_t)ld * cols * sizeof(double), c->stream));
            return full.view(0, 0, rows, cols);
        };
        auto put = [&](const double* h, const Mat& v, int c0, int rows, int cols) {
            DRE_HIP(hipMemcpy2DAsync(v.p + (size_t)c0 * v.ld, (size_t)v.ld * sizeof(double), h, (size_t)rows * sizeof(double), (size_t)rows * sizeof(double), (size_t)cols,
                                     hipMemcpyHostToDevice, c->stream));
        };
        auto get = [&](double* h, const Mat& v, int c0, int cols) {          // whole columns of the allocation, padding rows included
            if (h) DRE_HIP(hipMemcpyAsync(h, v.p + (size_t)c0 * v.ld, (size_t)v.ld * cols * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        };
        auto nan_arr = [&](size_t cnt) {
            DevArr<double> d(c, std::max<size_t>(cnt, 1));
            DRE_HIP(hipMemsetAsync(d.p, 0xFF, d.n * sizeof(double), c->stream));
            return d;
        };
        auto up = [&](double* d, const double* h, size_t cnt) { if (cnt) DRE_HIP(hipMemcpyAsync(d, h, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream)); };
        auto down = [&](double* h, const double* d, size_t cnt) { if (h && cnt) DRE_HIP(hipMemcpyAsync(h, d, cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream)); };
        if (!c->warm_tickets) {
            c->warm_tickets = std::make_shared<Buf>(c, 4 * sizeof(int));
            DRE_HIP(hipMemsetAsync(c->warm_tickets->p, 0, 4 * sizeof(int), c->stream));
        }
        int* const tickets = (int*)c->warm_tickets->p;
        auto finish = [&] {
            int ht[4] = {-1, -1, -1, -1};
            DRE_HIP(hipMemcpyAsync(ht, tickets, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            c->sync();
            if (p.ticket) { p.ticket[0] = ht[0]; p.ticket[1] = ht[1]; }
        };
        const int nstrip = rows_n ? ceil_div(n, 16) : 0, nslab = rows_n ? warm_project_slabs(n) : 0;
        if (st == DRE_WARM_PROBE_PROJECT || st == DRE_WARM_PROBE_Z || st == DRE_WARM_PROBE_ZAPPLY) {
            // the buffers of the callers: the basis buffer [Om | Q | Z], the right-hand block [Y_p, Y_f, W, Z, W_2], the slab with C behind the shares
            Mat QO = nan_mat(n, ldn, 32 + q + 16), YB = nan_mat(n, ldn, 64 + q), Z1 = nan_mat(n, ldn, 16);
            DevArr<double> slab = nan_arr((size_t)nslab * 256 + nstrip + 256);
            double* const Cw = slab.p + (size_t)nslab * 256 + nstrip;
            if (st == DRE_WARM_PROBE_PROJECT) {
                Mat Qv = QO.colsview(32, q), Yf = YB.colsview(16, 16), Pf(c, q, 16);
                put(p.Q, QO, 32, n, q); put(p.Yf, YB, 16, n, 16); up(Pf.p, p.Pf, (size_t)q * 16);
                warm_project(c, n, q, Qv, Yf, Pf, Z1, slab.p, tickets, Cw);
                get(p.Z1_out, Z1, 0, 16); down(p.Cw_out, Cw, 256); down(p.slab, slab.p, (size_t)nslab * 256);
            } else {
                put(p.Z1, Z1, 0, n, 16); up(Cw, p.Cw, 256);
                Mat Zb = QO.colsview(32 + q, 16), Zy = YB.colsview(32 + q, 16), W2 = YB.colsview(48 + q, 16);
                if (st == DRE_WARM_PROBE_Z) {
                    Mat Res = nan_mat(n, ldn, n);
                    put(p.Res, Res, 0, n, n);
                    warm_z(c, n, Z1, Cw, Res, Zb, Zy, W2);
                    get(p.W2, YB, 48 + q, 16);
                } else {
                    warm_zapply(c, n, Z1, Cw, Zb, Zy);
                }
                get(p.Zb, QO, 32 + q, 16); get(p.Zy, YB, 32 + q, 16);
            }
            finish();
            return;
        }
        if (st == DRE_WARM_PROBE_SMALL) {
            Mat Cc(c, m, 64 + q), Uc = nan_mat(m, m, qn), T = nan_mat(kl, kl, kl), Cp = nan_mat(m, m, 16), Mo = nan_mat(m, m, m), LT = nan_mat(m, m, m);
            up(Cc.p, p.Cc, (size_t)m * (64 + q));
            DevArr<double> parts(c, std::max(p.nparts, 1)), tols = nan_arr(12);
            up(parts.p, p.parts, (size_t)p.nparts);
            warm_small(c, q, m, kl, qn, Cc, p.nparts ? parts.p : nullptr, p.nparts, p.reltol, p.abstol, p.frac, p.budget_frac, tols.p, Uc, T, Cp, tickets + 1,
                       p.mode == 1 ? &Mo : nullptr, p.mode == 1 ? &LT : nullptr);
            down(p.tols, tols.p, 12); get(p.Uc, Uc, 0, qn); get(p.T, T, 0, kl); get(p.Cp, Cp, 0, 16); get(p.Mout, Mo, 0, m); get(p.LTout, LT, 0, m);
            finish();
            return;
        }
        if (st == DRE_WARM_PROBE_EIG) {
            Mat S(c, m, m), U = nan_mat(m, m, m);
            up(S.p, p.S, (size_t)m * m);
            warm_eig(c, m, S, U);
            get(p.U, U, 0, m);
            finish();
            return;
        }
        if (st == DRE_WARM_PROBE_FINISH) {
            const int rc = 16 * ceil_div(kl, 16);
            Mat B = nan_mat(n, ldn, q), Wk(c, q, kl), Yp = nan_mat(n, ldn, 16), Pp(c, q, 16), R = nan_mat(n, ldn, rc);
            put(p.Q, B, 0, n, q); up(Wk.p, p.Wk, (size_t)q * kl); put(p.Yp, Yp, 0, n, 16); up(Pp.p, p.Pp, (size_t)q * 16);
            DevArr<double> slab = nan_arr((size_t)nstrip), tols(c, 12);
            up(tols.p, p.tols_in, 12);
            warm_finish(c, n, q, kl, B, Wk, Yp, Pp, R, slab.p, tickets + 1, tols.p);
            get(p.R, R, 0, rc); down(p.tols, tols.p, 12); down(p.slab, slab.p, (size_t)nstrip);
            finish();
            return;
        }
        // CHAIN: the Jacobi form of the dense-X time loop's compression
        WarmChain w;
        const int mb = q + 16;
        w.n = n; w.qb = q; w.kl = kl; w.qn = qn;
        w.Res = nan_mat(n, ldn, n); w.QOc = nan_mat(n, ldn, 32 + 64 + 16); w.QOn = nan_mat(n, ldn, 32 + 64 + 16);
        put(p.Res, w.Res, 0, n, n); put(p.basis, w.QOc, 0, n, 32 + q);
        w.YB = nan_mat(n, ldn, 64 + q); w.Z1 = nan_mat(n, ldn, 16); w.Cc = nan_mat(mb, mb, 64 + q); w.Uc = nan_mat(mb, mb, qn); w.Cp = nan_mat(mb, mb, 16);
        w.Pf = nan_mat(q, q, 16); w.Tm = nan_mat(kl, kl, kl);
        DevArr<double> slab = nan_arr((size_t)nstrip * 256 + nstrip + 256), parts(c, std::max(p.nparts, 1)), tols = nan_arr(12);
        up(parts.p, p.parts, (size_t)p.nparts);
        w.slab = slab.p; w.tickets = tickets; w.tols = tols.p;
        w.parts = p.nparts ? parts.p : nullptr; w.nparts = p.nparts; w.reltol = p.reltol; w.abstol = p.abstol; w.frac = p.frac; w.bf = p.budget_frac;
        warm_chain_jacobi(c, w);
        get(p.R, w.QOn, 32, qn); get(p.basis_out, w.QOc, 0, 32 + q + 16); get(p.T, w.Tm, 0, kl); get(p.Uc, w.Uc, 0, qn); get(p.Cp, w.Cp, 0, 16);
        down(p.tols, tols.p, 12);
        finish();
    });
}
// ---- dre_adi_chain_probe: the dense-inverse ADI chain on caller-supplied operands (test and diagnostic surface) ----------------------------
// Every launch goes through adi_fast_build, adi_fast_pack_r, adi_fast_iter, adi_group_pack or adi_group_iter; the loops are those of adi_advance
// (engine.hip, fast branch) and of the dense-X time loop (dense_x.hip, group branch).
int dre_adi_chain_probe(dre_ctx* ctx, const dre_adi_chain_probe_args* args) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(args, "dre_adi_chain_probe: null argument");
        const dre_adi_chain_probe_args& p = *args;
        const bool group = p.kind == DRE_ADI_PROBE_GROUP, build_only = p.kind == DRE_ADI_PROBE_BUILD;
        DRE_REQUIRE(p.kind == DRE_ADI_PROBE_FAST || group || build_only, "dre_adi_chain_probe: unknown kind");
        const int n = p.n, k = p.k, m = group ? 0 : p.m, nit = p.nit, g = p.g;
        DRE_REQUIRE(n >= 1 && n <= 8192, "dre_adi_chain_probe: n must lie in 1 .. 8192");
        DRE_REQUIRE(p.nstack >= 1 && p.nstack <= 4096 && p.stacks, "dre_adi_chain_probe: stacks missing");
        DRE_REQUIRE(m >= 0 && m <= 4096 && (m == 0 || p.wks), "dre_adi_chain_probe: m must not be negative and needs wks");
        int mode = 0, nt = 1;
        if (!build_only) {
            DRE_REQUIRE(k >= 1, "dre_adi_chain_probe: k must be at least 1");
            DRE_REQUIRE(k <= (group ? ADI_GROUP_MAX_K : ADI_FAST_MAX_K), "dre_adi_chain_probe: residual too wide");
            DRE_REQUIRE(nit >= 1 && nit <= 480, "dre_adi_chain_probe: nit must lie in 1 .. 480 (ring of the norm history)");
            DRE_REQUIRE(p.ncyc >= 1 && p.mu && p.R0 && p.T, "dre_adi_chain_probe: cycle, R0 or T missing");
            DRE_REQUIRE(p.ld >= n + 2, "dre_adi_chain_probe: ld must be at least n + 2");
            DRE_REQUIRE(p.base_it >= 0 && p.base_it <= (1 << 30), "dre_adi_chain_probe: base_it");
            if (group) {
                DRE_REQUIRE(g >= 2 && g <= ADI_GROUP_MAX_G, "dre_adi_chain_probe: g must lie in 2 .. 6");
                DRE_REQUIRE(nit % g == 0, "dre_adi_chain_probe: nit must be a multiple of g");
                DRE_REQUIRE(p.ncyc % g == 0 && p.nstack == p.ncyc / g, "dre_adi_chain_probe: one group stack per start position of the cycle (ncyc / g)");
                const int ct = (k + 15) / 16;
                DRE_REQUIRE(g * ct * ((ct + 3) / 4) <= ADI_FAST_NWS - 1, "dre_adi_chain_probe: norm meeting point too small");
            } else {
                DRE_REQUIRE(p.cycle, "dre_adi_chain_probe: cycle missing");
                for (int i = 0; i < p.ncyc; ++i) DRE_REQUIRE(p.cycle[i] >= 0 && p.cycle[i] < p.nstack, "dre_adi_chain_probe: entry of cycle outside [0, nstack)");
                DRE_REQUIRE((p.mode == -1) == (p.nt == -1), "dre_adi_chain_probe: mode and nt are picked together");
                if (p.mode == -1) adi_fast_pick(n, k, &mode, &nt);
                else {
                    DRE_REQUIRE(p.mode == 0 || p.mode == 1, "dre_adi_chain_probe: mode must be 0 or 1");
                    DRE_REQUIRE(p.nt == 1 || p.nt == 2 || p.nt == 4, "dre_adi_chain_probe: nt must be 1, 2 or 4");
                    mode = p.mode; nt = p.nt;
                }
            }
        }
        // (the arguments are judged without a context, so that the refusals can be tested on a machine without a device)
        DRE_REQUIRE(ctx, "dre_adi_chain_probe: arguments accepted, context missing");
        Ctx* c = &ctx->c;
        const int nstrip = adi_fast_nstrip(n), kst = adi_fast_kst(n);
        const double nan = std::numeric_limits<double>::quiet_NaN();
        auto up = [&](const double* h, size_t cnt) {
            DevArr<double> d(c, std::max<size_t>(cnt, 1));
            if (cnt) DRE_HIP(hipMemcpyAsync(d.p, h, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
            return d;
        };
        auto nan_arr = [&](size_t cnt) {          // (all bits set is a NaN)
            DevArr<double> d(c, std::max<size_t>(cnt, 1));
            DRE_HIP(hipMemsetAsync(d.p, 0xFF, d.n * sizeof(double), c->stream));
            return d;
        };
        auto down = [&](double* h, const double* d, size_t cnt) { if (h && cnt) DRE_HIP(hipMemcpyAsync(h, d, cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream)); };
        // ---- the packed stacks ----
        const int srows = group ? 2 * g * n : 2 * n + m;
        const size_t pkd = group ? (size_t)2 * g * nstrip * kst * 64 : adi_fast_pack_doubles(n);
        DevArr<double> stacks_d = up(p.stacks, (size_t)p.nstack * srows * n);
        DevArr<double> wks_d = up(p.wks, m ? (size_t)p.nstack * 2 * n * m : 0);
        DevArr<double> packs_d = nan_arr((size_t)p.nstack * pkd);
        if (group) {
            for (int s = 0; s < p.nstack; ++s) adi_group_pack(c, n, 2 * g, stacks_d.p + (size_t)s * srows * n, srows, packs_d.p + (size_t)s * pkd);
        } else {
            std::vector<const double*> stacks, wks; std::vector<double*> outs;
            for (int s = 0; s < p.nstack; ++s) {
                stacks.push_back(stacks_d.p + (size_t)s * srows * n);
                wks.push_back(m && !(p.wks_null && p.wks_null[s]) ? wks_d.p + (size_t)s * 2 * n * m : nullptr);
                outs.push_back(packs_d.p + (size_t)s * pkd);
            }
            adi_fast_build(c, n, m, stacks, srows, wks, 2 * n, outs);
        }
        down(p.packs, packs_d.p, (size_t)p.nstack * pkd);
        if (build_only) { c->sync(); return; }
        // ---- control block, meeting point, buffers ----
        AdiState hst;
        std::memset(&hst, 0, sizeof(hst));
        hst.iters = p.base_it; hst.maxiters = p.maxiters; hst.abstol = p.abstol; hst.res_norm = nan;
        for (double& v : hst.norms) v = nan;
        DevArr<AdiState> st(c, 1);
        DRE_HIP(hipMemcpyAsync(st.p, &hst, sizeof(AdiState), hipMemcpyHostToDevice, c->stream));
        DevArr<double> nws(c, ADI_FAST_NWS);
        DRE_HIP(hipMemsetAsync(nws.p, 0, ADI_FAST_NWS * sizeof(double), c->stream));
        DevArr<double> R0 = up(p.R0, (size_t)n * k), Tm = up(p.T, (size_t)k * k);
        const int ld = p.ld;
        const size_t ring = (size_t)ld * k * (nit + 1);
        DevArr<double> Vall = nan_arr(ring), Rring = nan_arr(ring);
        const bool use_pk = group || mode == 0;
        const size_t rpd = adi_fast_rpack_doubles(n, k);
        DevArr<double> Rp0 = nan_arr(use_pk ? rpd : 1);                          // exactly one slot, like the time loop's
        DevArr<double> Rpk = nan_arr(use_pk ? rpd * (size_t)(nit + 1) : 1);
        DevArr<double> Gm = nan_arr((size_t)k * k * 2 * (group ? g : 1));
        if (use_pk) adi_fast_pack_r(c, n, k, R0.p, n, Rp0.p, st.p);
        const int base_it = p.base_it;
        if (group) {
            const int NG = nit / g;
            AdiGroupArgs ga;
            std::memset(&ga, 0, sizeof(ga));
            ga.n = n; ga.k = k; ga.nstrip = nstrip; ga.kst = kst; ga.g = g;
            ga.ldr = ld; ga.rpd = rpd; ga.ldv = ld;
            ga.T = Tm.p; ga.ldt = k; ga.alpha = p.alpha; ga.st = st.p; ga.nws = nws.p;
            for (int L = 0; L <= NG + 1; ++L) {
                ga.do_strips = L < NG ? 1 : 0;
                if (L < NG) {
                    ga.Gpack = packs_d.p + (size_t)(((L * g) % p.ncyc) / g) * pkd;
                    ga.Rpc = L == 0 ? Rp0.p : Rpk.p + (size_t)(L * g) * rpd;
                    ga.Rring = Rring.p + (size_t)(L * g) * k * ld;
                    ga.Rpk = Rpk.p + (size_t)(L * g + 1) * rpd;
                    ga.V = Vall.p + (size_t)(L * g * k) * ld;
                }
                // Gram matrices of the residuals launch L - 1 produced; norms + decisions for those of launch L - 2
                ga.n_prev = (L >= 1 && L <= NG) ? g : 0;
                ga.Rp_prev = ga.n_prev ? Rpk.p + (size_t)((L - 1) * g + 1) * rpd : nullptr;
                ga.G_prev = Gm.p + (size_t)(L & 1) * g * k * k;
                ga.n_prev2 = L >= 2 ? g : 0;
                ga.G_prev2 = Gm.p + (size_t)((L - 1) & 1) * g * k * k;
                ga.it0_prev2 = base_it + (L - 2) * g + 1;
                adi_group_iter(c, ga);
            }
        } else {
            AdiFastArgs a;
            std::memset(&a, 0, sizeof(a));
            a.n = n; a.k = k; a.nstrip = nstrip; a.kst = kst; a.mode = mode; a.nt = nt;
            a.T = Tm.p; a.ldt = k; a.tdiag = p.tdiag ? 1 : 0; a.alpha = p.alpha; a.st = st.p; a.nws = nws.p;
            for (int j = 1; j <= nit; ++j) {
                const int pos = (j - 1) % p.ncyc;
                a.Apack = packs_d.p + (size_t)p.cycle[pos] * pkd;
                if (j == 1) { a.Rcur = R0.p; a.ldr = n; } else { a.Rcur = Rring.p + (size_t)(j - 2) * k * ld; a.ldr = ld; }
                a.Rnext = Rring.p + (size_t)(j - 1) * k * ld; a.ldr_next = ld;
                a.Rpc = use_pk ? (j == 1 ? Rp0.p : Rpk.p + (size_t)(j - 1) * rpd) : nullptr;
                a.Rpn = use_pk ? Rpk.p + (size_t)j * rpd : nullptr;
                a.V = Vall.p + (size_t)(j - 1) * k * ld; a.ldv = ld;
                a.two_mu = 2.0 * p.mu[pos];
                const int it = base_it + j;                                 // shifts consumed after this iteration
                a.G_prev = j >= 2 ? Gm.p + (size_t)((it - 1) & 1) * k * k : nullptr;
                a.G_prev2 = j >= 3 ? Gm.p + (size_t)((it - 2) & 1) * k * k : nullptr;
                a.it_prev2 = it - 2; a.do_strips = 1;
                adi_fast_iter(c, a);
            }
            {   // drain the norm pipeline: Gram matrix of the last residual, decisions for the last two iterations
                const int it = base_it + nit;
                a.do_strips = 0; a.Apack = nullptr; a.Rnext = nullptr; a.V = nullptr;
                a.Rpc = use_pk ? Rpk.p + (size_t)nit * rpd : nullptr; a.Rpn = nullptr;
                a.Rcur = Rring.p + (size_t)(nit - 1) * k * ld; a.ldr = ld;
                a.G_prev = Gm.p + (size_t)(it & 1) * k * k;
                a.G_prev2 = nit >= 2 ? Gm.p + (size_t)((it - 1) & 1) * k * k : nullptr;
                a.it_prev2 = it - 1;
                adi_fast_iter(c, a);
                a.G_prev = nullptr;
                a.G_prev2 = Gm.p + (size_t)(it & 1) * k * k;
                a.it_prev2 = it;
                adi_fast_iter(c, a);
            }
        }
        DRE_HIP(hipMemcpyAsync(&hst, st.p, sizeof(AdiState), hipMemcpyDeviceToHost, c->stream));
        down(p.V, Vall.p, ring);
        down(p.R, Rring.p, ring);
        down(p.G, Gm.p, (size_t)k * k * 2 * (group ? g : 1));
        if (p.Rp) {
            if (use_pk) { down(p.Rp, Rp0.p, rpd); down(p.Rp + rpd, Rpk.p + rpd, rpd * (size_t)nit); }
            else for (size_t i = 0; i < rpd * (size_t)(nit + 1); ++i) p.Rp[i] = nan;
        }
        c->sync();
        if (p.state_i) { p.state_i[0] = hst.iters; p.state_i[1] = hst.done; p.state_i[2] = mode; p.state_i[3] = nt; }
        if (p.state_d) { p.state_d[0] = hst.res_norm; p.state_d[1] = hst.abstol; std::memcpy(p.state_d + 2, hst.norms, sizeof(hst.norms)); }
    });
}
int dre_sym_eig_jacobi(dre_ctx* ctx, const dre_dense* S, double tol, dre_dense** values, dre_dense** vectors, int64_t* stats) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(S && values && vectors, "dre_sym_eig_jacobi: null argument");
        BjStats bs;
        SymEig e = sym_eig_jacobi(c, S->m, tol, &bs);
        std::vector<int> ids(e.j);
        for (int i = 0; i < e.j; ++i) ids[i] = i;
        std::sort(ids.begin(), ids.end(), [&](int a, int b) { return e.w[a] < e.w[b]; });
        std::vector<double> w(e.j);
        for (int i = 0; i < e.j; ++i) w[i] = e.w[ids[i]];
        auto* V = new dre_dense();
        V->m = sym_eig_backtransform(c, e, ids);
        auto* W = new dre_dense();
        W->m = Mat(c, e.j, 1);
        if (e.j) {
            DRE_HIP(hipMemcpyAsync(W->m.p, w.data(), e.j * sizeof(double), hipMemcpyHostToDevice, c->stream));
            DRE_HIP(hipStreamSynchronize(c->stream));
        }
        if (stats) { stats[0] = bs.sweeps; stats[1] = bs.rounds; }
        *values = W; *vectors = V;
    });
}
int dre_shift_factor(dre_ctx* ctx, const dre_pencil* p, double cA, double cE_re, double cE_im, dre_factor** out) {
    return guarded(ctx, [&] {
        const Pencil& P = *p->p;
        DRE_REQUIRE(P.has_device, "pencil was created host-only");
        auto* f = new dre_factor();
        f->pen = p;
        f->is_cplx = cE_im != 0.0;
        try {
            if (f->is_cplx) { mf_factor<cplx>(&ctx->c, P, P.valAt.p, P.valEt.p, cplx{cA, 0.0}, cplx{cE_re, cE_im}, f->fc); mf_check(&ctx->c, f->fc); }
            else { mf_factor<double>(&ctx->c, P, P.valAt.p, P.valEt.p, cA, cE_re, f->fr); mf_check(&ctx->c, f->fr); }
        } catch (...) { delete f; throw; }
        *out = f;
    });
}

__global__ void k_split_cplx(int rows, int cols, const cplx* __restrict__ src, int lds_, double* __restrict__ re, int ldr,
                             double* __restrict__ im, int ldi) {
    size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)rows * cols) return;
    int r = id % rows, c = id / rows;
    cplx z = src[r + (size_t)c * lds_];
    re[r + (size_t)c * ldr] = z.re;
    im[r + (size_t)c * ldi] = z.im;
}
__global__ void k_make_cplx(int rows, int cols, const double* __restrict__ src, int lds_, cplx* __restrict__ dst, int ldd) {
    size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)rows * cols) return;
    int r = id % rows, c = id / rows;
    dst[r + (size_t)c * ldd] = {src[r + (size_t)c * lds_], 0.0};
}

int dre_shift_solve(dre_ctx* ctx, const dre_factor* f, const dre_dense* B, dre_dense** X_re, dre_dense** X_im) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const Pencil& P = *f->pen->p;
        Mat Bs = to_solver_order(c, f->pen, B->m);
        const int n = P.n, k = Bs.cols;
        if (!f->is_cplx) {
            Mat W(c, n, k);
            copy_mat(c, Bs, W);
            mf_solve<double>(c, P, f->fr, W.p, W.ld, k);
            auto* X = new dre_dense();
            X->m = Mat(c, n, k);
            Mat Xu = to_user_order(c, f->pen, W);
            copy_mat(c, Xu, X->m);
            *X_re = X;
            if (X_im) *X_im = nullptr;
        } else {
            DRE_REQUIRE(X_im != nullptr, "complex factor needs an imaginary output");
            DevArr<cplx> W(c, (size_t)n * std::max(k, 1));
            size_t tot = (size_t)n * k;
            if (tot) hipLaunchKernelGGL(k_make_cplx, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, n, k, Bs.p, Bs.ld, W.p, n);
            mf_solve<cplx>(c, P, f->fc, W.p, n, k);
            Mat re(c, n, k), im(c, n, k);
            if (tot) hipLaunchKernelGGL(k_split_cplx, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, n, k, W.p, n, re.p, re.ld, im.p, im.ld);
            auto* Xr = new dre_dense(); auto* Xi = new dre_dense();
            Xr->m = Mat(c, n, k); Xi->m = Mat(c, n, k);
            Mat ru = to_user_order(c, f->pen, re), iu = to_user_order(c, f->pen, im);
            copy_mat(c, ru, Xr->m); copy_mat(c, iu, Xi->m);
            c->sync();
            *X_re = Xr; *X_im = Xi;
        }
    });
}
int dre_shift_solve_smw(dre_ctx* ctx, const dre_factor* f, double alpha, const dre_dense* U, const dre_dense* Vt, const dre_dense* B,
                        dre_dense** X_re, dre_dense** X_im) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const Pencil& P = *f->pen->p;
        DRE_REQUIRE(U && Vt && B && X_re, "dre_shift_solve_smw: null argument");
        Mat Us = to_solver_order(c, f->pen, U->m), Vs = to_solver_order(c, f->pen, Vt->m), Bs = to_solver_order(c, f->pen, B->m);
        if (!f->is_cplx) {
            Mat X = smw_solve(c, P, f->fr, alpha, Us, Vs, Bs);
            auto* Xr = new dre_dense();
            Xr->m = Mat(c, P.n, Bs.cols);
            Mat Xu = to_user_order(c, f->pen, X);
            copy_mat(c, Xu, Xr->m);
            c->sync();
            *X_re = Xr;
            if (X_im) *X_im = nullptr;
        } else {
            DRE_REQUIRE(X_im != nullptr, "complex factor needs an imaginary output");
            Mat re, im;
            smw_solve(c, P, f->fc, alpha, Us, Vs, Bs, re, im);
            auto* Xr = new dre_dense(); auto* Xi = new dre_dense();
            Xr->m = Mat(c, P.n, Bs.cols); Xi->m = Mat(c, P.n, Bs.cols);
            Mat ru = to_user_order(c, f->pen, re), iu = to_user_order(c, f->pen, im);
            copy_mat(c, ru, Xr->m); copy_mat(c, iu, Xi->m);
            c->sync();
            *X_re = Xr; *X_im = Xi;
        }
    });
}
int dre_factor_growth(dre_ctx* ctx, const dre_factor* f, double* growth) {
    return guarded(ctx, [&] { *growth = f->is_cplx ? mf_check(&ctx->c, f->fc) : mf_check(&ctx->c, f->fr); });
}
int dre_factor_perturbed(dre_ctx* ctx, const dre_factor* f, int64_t* count) {
    return guarded(ctx, [&] {
        if (f->is_cplx) { if (f->fc.nperturbed < 0) mf_check(&ctx->c, f->fc); *count = f->fc.nperturbed; }
        else { if (f->fr.nperturbed < 0) mf_check(&ctx->c, f->fr); *count = f->fr.nperturbed; }
    });
}
int dre_factor_free(dre_ctx*, dre_factor* f) { delete f; return DRE_OK; }

// ---- LDLt --------------------------------------------------------------------------------------
int dre_ldlt_create(dre_ctx* ctx, const dre_pencil* p, const dre_dense* L, const dre_dense* D, double alpha, dre_ldlt** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(D->m.rows == D->m.cols && D->m.rows == L->m.cols, "lowrank: D must be k x k with k = size(L, 2)");
        Mat Ls = to_solver_order(c, p, L->m);
        if (!p) { Ls = Mat(c, L->m.rows, L->m.cols); copy_mat(c, L->m, Ls); }
        Mat Dc(c, D->m.rows, D->m.cols);
        copy_mat(c, D->m, Dc);
        auto* h = new dre_ldlt();
        h->x = ldlt_make(c, L->m.rows, Ls, Dc, alpha, false);
        h->pen = p;
        *out = h;
    });
}
int dre_ldlt_zero(dre_ctx* ctx, const dre_pencil* p, int n, dre_ldlt** out) {
    return guarded(ctx, [&] { auto* h = new dre_ldlt(); h->x = ldlt_zero(n); h->pen = p; *out = h; });
}
int dre_ldlt_free(dre_ctx*, dre_ldlt* x) { delete x; return DRE_OK; }
int dre_ldlt_info(const dre_ldlt* x, int* n, int* rank, int* nblocks) {
    *n = x->x->n; *rank = x->x->rank(); *nblocks = (int)x->x->blocks.size();
    return DRE_OK;
}
int dre_ldlt_add(dre_ctx* ctx, const dre_ldlt* a, const dre_ldlt* b, dre_ldlt** out) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(a->pen == b->pen, "LDLt operands live in different orderings");
        auto* h = new dre_ldlt();
        h->x = ldlt_add(a->x, b->x);
        if (h->x.get() == a->x.get() || h->x.get() == b->x.get()) h->x = std::make_shared<LDLt>(*h->x);
        h->pen = a->pen;
        *out = h;
    });
}
int dre_ldlt_scale(dre_ctx* ctx, const dre_ldlt* a, double alpha, dre_ldlt** out) {
    return guarded(ctx, [&] { auto* h = new dre_ldlt(); h->x = ldlt_scale(a->x, alpha); h->pen = a->pen; *out = h; });
}
int dre_ldlt_concatenate(dre_ctx* ctx, dre_ldlt* x) { return guarded(ctx, [&] { ldlt_concatenate(&ctx->c, *x->x); }); }
int dre_ldlt_compress(dre_ctx* ctx, dre_ldlt* x) { return guarded(ctx, [&] { ldlt_compress(&ctx->c, *x->x); }); }
int dre_ldlt_compress_tol(dre_ctx* ctx, dre_ldlt* x, double abs_tol) {
    return guarded(ctx, [&] { ldlt_compress(&ctx->c, *x->x, 4.0, false, abs_tol > 0.0 ? abs_tol : -1.0); });
}
int dre_ldlt_compress_fast(dre_ctx* ctx, dre_ldlt* x) { return guarded(ctx, [&] { ldlt_compress(&ctx->c, *x->x, 4.0, false, -1.0); }); }
int dre_ldlt_canonicalize(dre_ctx* ctx, dre_ldlt* x) {
    return guarded(ctx, [&] {
        LDLt& X = *x->x;
        if (X.blocks.size() > 1 || (X.blocks.size() == 1 && !X.blocks[0].diag && X.blocks[0].L.cols > 0)) ldlt_compress(&ctx->c, X, 4.0, true);
    });
}
int dre_ldlt_norm(dre_ctx* ctx, dre_ldlt* x, double* out) { return guarded(ctx, [&] { *out = ldlt_norm_accurate(&ctx->c, *x->x); }); }
int dre_ldlt_destructure(dre_ctx* ctx, dre_ldlt* x, double* alpha, double* Lh, int ldl, double* Dh, int ldd) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        ldlt_destructure(c, *x->x);
        const LBlock& b = x->x->blocks[0];
        if (alpha) *alpha = b.alpha;
        if (Lh) { Mat Lu = to_user_order(c, x->pen, b.L); download_mat(c, Lu, Lh, ldl); }
        if (Dh) download_mat(c, b.D, Dh, ldd);
    });
}

// ---- GALE / ADI --------------------------------------------------------------------------------
int dre_adi_default_options(dre_adi_options* o) {
    std::memset(o, 0, sizeof(*o));
    o->maxiters = 100; o->reltol = -1.0; o->abstol = -1.0; o->ignore_initial_guess = 0; o->compression_interval = 10;
    o->compression = 1; o->shift_kind = 1; o->n_history = 2; o->nshifts = 0; o->shifts_re = nullptr; o->shifts_im = nullptr;
    o->compress_tolfac = 4.0;
    o->compress_exact = 0;
    o->heuristic_kplus = 0; o->heuristic_kminus = 0;
    o->shift_fn = nullptr; o->shift_user = nullptr;
    return DRE_OK;
}
static AdiOptions convert_options(const dre_adi_options* o) {
    AdiOptions a;
    if (!o) return a;
    a.maxiters = o->maxiters; a.reltol = o->reltol; a.abstol = o->abstol; a.ignore_initial_guess = o->ignore_initial_guess != 0;
    a.compression_interval = o->compression_interval; a.compression = o->compression != 0;
    a.compress_tolfac = o->compress_tolfac > 0 ? o->compress_tolfac : 4.0;
    a.compress_exact = o->compress_exact != 0;
    a.inner_solve = o->inner_solve; a.inner_user = o->inner_user;
    if (o->shift_kind == 0) {
        a.shifts.kind = ShiftSpec::CYCLIC;
        DRE_REQUIRE(o->nshifts > 0 && o->shifts_re, "Cyclic shifts need at least one value");
        for (int i = 0; i < o->nshifts; ++i) a.shifts.values.emplace_back(o->shifts_re[i], o->shifts_im ? o->shifts_im[i] : 0.0);
    } else if (o->shift_kind == 2) {
        a.shifts.kind = ShiftSpec::HEURISTIC;
        DRE_REQUIRE(o->nshifts > 0 && o->heuristic_kplus > 0 && o->heuristic_kminus > 0, "Heuristic(nshifts, k+, k-) must be positive");
        a.shifts.h_nshifts = o->nshifts; a.shifts.h_kplus = o->heuristic_kplus; a.shifts.h_kminus = o->heuristic_kminus;
    } else if (o->shift_kind == 3) {
        a.shifts.kind = ShiftSpec::USER;
        DRE_REQUIRE(o->shift_fn != nullptr, "shift_kind 3 (user-defined strategy) needs shift_fn");
        DRE_REQUIRE(o->n_history > 0, "shift_kind 3: n_history must be positive");
        a.shifts.user_fn = o->shift_fn; a.shifts.user_data = o->shift_user; a.shifts.n_history = o->n_history;
    } else {
        a.shifts.kind = ShiftSpec::PROJECTION;
        DRE_REQUIRE(o->n_history > 0 && o->n_history % 2 == 0, "History must be even");   // projection.jl:28-32
        a.shifts.n_history = o->n_history;
    }
    return a;
}
static std::atomic<uint64_t> g_tag_counter{1ull << 40};     // operator identities for the factor caches (unique across threads)
static GaleOperator make_operator(Ctx* c, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt) {
    const Pencil& P = *p->p;
    DRE_REQUIRE(P.has_device, "pencil was created host-only");
    GaleOperator op;
    op.P = &P;
    op.valFt = DevArr<double>(c, P.nnz);
    vals_axpby(c, P.nnz, cA, P.valAt.p, cE, P.valEt.p, op.valFt.p);
    op.tag = g_tag_counter++;
    op.cA = cA; op.cE = cE;
    if (U && Vt) {
        DRE_REQUIRE(U->m.rows == P.n && Vt->m.rows == P.n && U->m.cols == Vt->m.cols, "low-rank factors must be n x m");
        op.has_lr = true; op.alpha = lr_alpha;
        op.U = to_solver_order(c, p, U->m);
        op.Vt = to_solver_order(c, p, Vt->m);
    }
    return op;
}
// The sketch of a wide factor (ldlt.hip sketch_compress) is chosen from what earlier compressions at the same order left in the context:
// the rank hint and the fallback counters.  A solve entered through the ABI starts from a clean slate, so that two identical calls return
// identical bits whatever ran on the context before (the explicit compression entry dre_ldlt_compress_fast keeps the history: that is
// its documented behaviour).
static void reset_sketch_history(Ctx* c, int n) {
    const long skey = -(4000000000L + (long)n);
    c->band_hint.erase(skey); c->band_hint.erase(skey - 1); c->band_hint.erase(skey - 2);
}
int dre_gale_solve(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                   dre_ldlt* C, const dre_ldlt* X0, const dre_adi_options* opt, dre_adi_result** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(C->pen == p && (!X0 || X0->pen == p), "LDLt operands must be created with the same pencil");
        GaleOperator op = make_operator(c, p, cA, cE, lr_alpha, U, Vt);
        AdiOptions ao = convert_options(opt);
        auto* r = new dre_adi_result();
        r->pen = p;
        reset_sketch_history(c, p->p->n);
        try { r->r = adi_solve(c, op, *C->x, X0 ? X0->x : nullptr, ao, nullptr); } catch (...) { delete r; throw; }
        *out = r;
    });
}
// ---- stepwise protocol: init / step! / isdone / solve! on the solver object (src/lyapunov/adi.jl:29-141) -------------------------
struct dre_adi_solver {
    std::shared_ptr<AdiRun> run;
    const dre_pencil* pen = nullptr;
};
int dre_adi_init(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                 dre_ldlt* C, const dre_ldlt* X0, const dre_adi_options* opt, dre_adi_solver** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(C->pen == p && (!X0 || X0->pen == p), "LDLt operands must be created with the same pencil");
        GaleOperator op = make_operator(c, p, cA, cE, lr_alpha, U, Vt);
        AdiOptions ao = convert_options(opt);
        auto* s = new dre_adi_solver();
        s->pen = p;
        reset_sketch_history(c, p->p->n);
        try { s->run = adi_begin(c, op, *C->x, X0 ? X0->x : nullptr, ao, nullptr); } catch (...) { delete s; throw; }
        *out = s;
    });
}
int dre_adi_step(dre_ctx* ctx, dre_adi_solver* s) { return guarded(ctx, [&] { adi_advance(*s->run, 1); }); }
int dre_adi_solve(dre_ctx* ctx, dre_adi_solver* s) {
    return guarded(ctx, [&] { while (!adi_isdone(*s->run)) adi_advance(*s->run, 1 << 30); });
}
int dre_adi_isdone(const dre_adi_solver* s, int* done) { *done = adi_isdone(*s->run) ? 1 : 0; return DRE_OK; }
int dre_adi_state(const dre_adi_solver* s, int64_t* iters, double* res_norm, double* abstol) {
    int it = 0; double rn = 0, at = 0;
    adi_peek(*s->run, &it, &rn, &at);
    if (iters) *iters = it;
    if (res_norm) *res_norm = rn;
    if (abstol) *abstol = at;
    return DRE_OK;
}
int dre_adi_shifts(const dre_adi_solver* s, int64_t from, int64_t* count, double* re, double* im) {
    auto v = adi_shifts_since(*s->run, (int)from);
    if (count) *count = (int64_t)v.size();
    for (size_t i = 0; i < v.size(); ++i) { if (re) re[i] = v[i].real(); if (im) im[i] = v[i].imag(); }
    return DRE_OK;
}
int dre_adi_snapshot(dre_ctx* ctx, dre_adi_solver* s, dre_ldlt** X, dre_ldlt** residual) {
    return guarded(ctx, [&] {
        LDLtP x, r;
        adi_snapshot(*s->run, X ? &x : nullptr, residual ? &r : nullptr);
        if (X) { auto* h = new dre_ldlt(); h->x = x; h->pen = s->pen; *X = h; }
        if (residual) { auto* h = new dre_ldlt(); h->x = r; h->pen = s->pen; *residual = h; }
    });
}
int dre_adi_finish(dre_ctx* ctx, dre_adi_solver* s, dre_adi_result** out) {
    return guarded(ctx, [&] {
        auto* r = new dre_adi_result();
        r->pen = s->pen;
        try { r->r = adi_finish(*s->run); } catch (...) { delete r; throw; }
        *out = r;
    });
}
int dre_adi_free(dre_adi_solver* s) { delete s; return DRE_OK; }

int dre_heuristic_ritz(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                       int kplus, int kminus, double* plus_re, double* plus_im, double* minus_re, double* minus_im) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        GaleOperator op = make_operator(c, p, cA, cE, lr_alpha, U, Vt);
        std::vector<std::complex<double>> rp, rm;
        heuristic_ritz(c, op, kplus, kminus, rp, rm);
        for (int i = 0; i < kplus; ++i) { plus_re[i] = rp[i].real(); plus_im[i] = rp[i].imag(); }
        for (int i = 0; i < kminus; ++i) { minus_re[i] = rm[i].real(); minus_im[i] = rm[i].imag(); }
    });
}
int dre_gale_residual(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                      dre_ldlt* C, dre_ldlt* X, dre_ldlt** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        GaleOperator op = make_operator(c, p, cA, cE, lr_alpha, U, Vt);
        auto* h = new dre_ldlt();
        h->pen = p;
        try { h->x = gale_residual(c, op, *C->x, X ? X->x : nullptr); } catch (...) { delete h; throw; }
        *out = h;
    });
}
int dre_ldlt_dot(dre_ctx* ctx, const dre_ldlt* a, const dre_ldlt* b, double* out) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(a->pen == b->pen, "dot: both operands must be created with the same pencil (same row ordering)");
        *out = ldlt_dot(&ctx->c, *a->x, *b->x);
    });
}
int dre_gale_apply(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                   const dre_ldlt* X, dre_ldlt** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(X->pen == p, "LDLt operand must be created with the same pencil");
        GaleOperator op = make_operator(c, p, cA, cE, lr_alpha, U, Vt);
        auto* h = new dre_ldlt();
        h->pen = p;
        try { h->x = lyapunov_apply(c, op, X->x); } catch (...) { delete h; throw; }
        *out = h;
    });
}
int dre_gare_residual(dre_ctx* ctx, const dre_pencil* p, dre_ldlt* X, const dre_dense* Ct, const dre_dense* S, double gamma, const dre_dense* B,
                      const dre_dense* Rinv, double beta, dre_ldlt** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(X->pen == p, "LDLt operand must be created with the same pencil");
        DRE_REQUIRE(Ct->m.rows == p->p->n && B->m.rows == p->p->n && S->m.rows == Ct->m.cols && Rinv->m.rows == B->m.cols, "dre_gare_residual: shape mismatch");
        Mat Cs = to_solver_order(c, p, Ct->m), Bs = to_solver_order(c, p, B->m);
        auto* h = new dre_ldlt();
        h->pen = p;
        try { h->x = gare_residual_dev(c, *p->p, *X->x, Cs, S->m, gamma, Bs, Rinv->m, beta); } catch (...) { delete h; throw; }
        *out = h;
    });
}
int dre_ldlt_feedback(dre_ctx* ctx, const dre_pencil* p, dre_ldlt* X, const dre_dense* B, dre_dense** Kt) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(X->pen == p && B->m.rows == p->p->n, "dre_ldlt_feedback: operand mismatch");
        Mat Bs = to_solver_order(c, p, B->m);
        Mat Ks = ldlt_feedback_dev(c, *p->p, *X->x, Bs);
        auto* K = new dre_dense();
        Mat Ku = to_user_order(c, p, Ks);
        K->m = Mat(c, Ku.rows, Ku.cols);
        copy_mat(c, Ku, K->m);
        *Kt = K;
    });
}
int dre_adi_result_info(const dre_adi_result* r, int64_t* info, double* dinfo) {
    info[0] = r->r.iters; info[1] = r->r.converged; info[2] = r->r.warnings; info[3] = (int64_t)r->r.norms.size(); info[4] = r->r.rhs_cols;
    dinfo[0] = r->r.res_norm; dinfo[1] = r->r.abstol; dinfo[2] = r->r.initial_norm;
    return DRE_OK;
}
int dre_adi_result_history(const dre_adi_result* r, double* norms, int32_t* norm_iters, double* sre, double* sim) {
    for (size_t i = 0; i < r->r.norms.size(); ++i) { if (norms) norms[i] = r->r.norms[i]; if (norm_iters) norm_iters[i] = r->r.norm_iters[i]; }
    for (size_t i = 0; i < r->r.shifts.size(); ++i) { if (sre) sre[i] = r->r.shifts[i].real(); if (sim) sim[i] = r->r.shifts[i].imag(); }
    return DRE_OK;
}
int dre_adi_result_take_x(dre_adi_result* r, dre_ldlt** X) {
    auto* h = new dre_ldlt(); h->x = r->r.X; h->pen = r->pen; *X = h; return DRE_OK;
}
int dre_adi_result_take_residual(dre_adi_result* r, dre_ldlt** R) {
    auto* h = new dre_ldlt(); h->x = r->r.residual; h->pen = r->pen; *R = h; return DRE_OK;
}
int dre_adi_result_free(dre_adi_result* r) { delete r; return DRE_OK; }

// ---- communicator (RCCL over xGMI, comm.hip) ----------------------------------------------------
int dre_comm_unique_id(dre_ctx* ctx, void* id128) { return guarded(ctx, [&] { DRE_REQUIRE(id128, "null id buffer"); comm_unique_id(id128); }); }
int dre_comm_init(dre_ctx* ctx, int nranks, int rank, const void* id128) {
    return guarded(ctx, [&] {
        const int emu = ctx->c.comm ? ctx->c.comm->emulate : 0;
        ctx->c.comm = comm_init(&ctx->c, nranks, rank, id128);
        ctx->c.comm->emulate = emu;
    });
}
int dre_comm_init_host(dre_ctx* ctx, int nranks, int rank, dre_comm_allgather_fn allgather, dre_comm_allreduce_fn allreduce, void* user) {
    return guarded(ctx, [&] {
        const int emu = ctx->c.comm ? ctx->c.comm->emulate : 0;
        ctx->c.comm = comm_init_host(&ctx->c, nranks, rank, allgather, allreduce, user);
        ctx->c.comm->emulate = emu;
    });
}
int dre_comm_free(dre_ctx* ctx) {
    return guarded(ctx, [&] { if (ctx->c.comm) { DRE_HIP(hipStreamSynchronize(ctx->c.stream)); ctx->c.comm.reset(); } });
}
int dre_comm_info(dre_ctx* ctx, int64_t* info) {
    const Comm* c = ctx->c.comm.get();
    info[0] = c ? c->nranks : 1; info[1] = c ? c->rank : 0; info[2] = c ? (int64_t)c->ncalls : 0;
    info[3] = c ? (int64_t)c->bytes_gathered : 0; info[4] = c ? (int64_t)c->bytes_reduced : 0; info[5] = c ? c->emulate : 0;
    return DRE_OK;
}
int dre_comm_allgather(dre_ctx* ctx, const void* send_dev, void* recv_dev, size_t count) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(ctx->c.comm, "dre_comm_allgather: no communicator (dre_comm_init)");
        comm_allgather(&ctx->c, *ctx->c.comm, (const double*)send_dev, (double*)recv_dev, count);
    });
}
int dre_comm_allreduce_sum(dre_ctx* ctx, void* buf_dev, size_t count) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(ctx->c.comm, "dre_comm_allreduce_sum: no communicator (dre_comm_init)");
        comm_allreduce_sum(&ctx->c, *ctx->c.comm, (double*)buf_dev, count);
    });
}

// ---- GDRE --------------------------------------------------------------------------------------
int dre_gdre_solve(dre_ctx* ctx, const dre_pencil* p, const dre_dense* B, const dre_dense* C, dre_ldlt* X0, double t0, double tf,
                   double dt, int order, int save_state, const dre_adi_options* opt, dre_gdre_result** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const Pencil& P = *p->p;
        DRE_REQUIRE(P.has_device, "pencil was created host-only");
        DRE_REQUIRE(X0->pen == p, "X0 must be created with the same pencil");
        DRE_REQUIRE(B->m.rows == P.n && C->m.cols == P.n, "B must be n x m and C must be q x n");
        GdreProblem prob;
        prob.P = &P;
        prob.B = to_solver_order(c, p, B->m);
        Mat Ct(c, P.n, C->m.rows);
        transpose_mat(c, C->m, Ct);
        prob.Ct = to_solver_order(c, p, Ct);
        prob.X0 = X0->x;
        prob.t0 = t0; prob.tf = tf;
        AdiOptions ao = convert_options(opt);
        auto* r = new dre_gdre_result();
        r->pen = p; r->m = B->m.cols;
        reset_sketch_history(c, p->p->n);
        try { r->r = gdre_solve(c, prob, order, dt, save_state != 0, ao); } catch (...) { delete r; throw; }
        *out = r;
    });
}
int dre_gdre_result_info(const dre_gdre_result* r, int64_t* info) {
    if (r->dense) {
        info[0] = (int64_t)r->r.t.size(); info[1] = (int64_t)r->Xd.size(); info[2] = 0; info[3] = 0;
        info[4] = (int64_t)r->solves.size(); info[5] = r->m; info[6] = r->n;
        return DRE_OK;
    }
    info[0] = (int64_t)r->r.t.size(); info[1] = (int64_t)r->r.X.size(); info[2] = r->r.adi_iters; info[3] = r->r.nfactor;
    info[4] = (int64_t)r->r.gale.size(); info[5] = r->m; info[6] = r->pen->p->n;
    return DRE_OK;
}
int dre_gdre_result_times(const dre_gdre_result* r, double* t) {
    std::memcpy(t, r->r.t.data(), r->r.t.size() * sizeof(double));
    return DRE_OK;
}
int dre_gdre_result_K(dre_ctx* ctx, const dre_gdre_result* r, int i, double* K_host, int ld) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(i >= 0 && i < (int)r->r.Kt.size(), "K index out of range");
        Mat Ktu = to_user_order(c, r->pen, r->r.Kt[i]);      // n x m
        Mat K(c, Ktu.cols, Ktu.rows);
        transpose_mat(c, Ktu, K);
        download_mat(c, K, K_host, ld);
    });
}
// K(t_i)(j, old) = Kt_i(iperm[old], j) for up to 64 time points per launch (the table of factors travels as kernel arguments): the whole
// trajectory leaves the solver ordering in one pass instead of a permutation and a transposition launch per time point
struct KTrajBatch { const double* Kt[64]; int ld[64]; };
__global__ void k_traj_export(int n, int m, const int* __restrict__ iperm, KTrajBatch bt, double* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * m) return;
    const int j = idx % m, old = idx / m;
    const int src = iperm ? iperm[old] : old;
    out[(size_t)blockIdx.y * n * m + idx] = bt.Kt[blockIdx.y][src + (size_t)j * bt.ld[blockIdx.y]];
}
static void export_trajectory(Ctx* c, const dre_gdre_result* r, double* K_dev) {
    const int nt = (int)r->r.Kt.size();
    if (nt == 0) return;
    const int n = r->r.Kt[0].rows, m = r->r.Kt[0].cols;
    if (n * m == 0) return;
    for (int i0 = 0; i0 < nt; i0 += 64) {
        KTrajBatch bt;
        const int nb = std::min(64, nt - i0);
        for (int i = 0; i < 64; ++i) {
            const Mat& K = r->r.Kt[(size_t)(i0 + std::min(i, nb - 1))];
            DRE_REQUIRE(K.rows == n && K.cols == m, "K trajectory: inconsistent shapes");
            bt.Kt[i] = K.p; bt.ld[i] = K.ld;
        }
        hipLaunchKernelGGL(k_traj_export, dim3((unsigned)((n * m + 255) / 256), (unsigned)nb), dim3(256), 0, c->stream, n, m,
                           r->pen ? (const int*)r->pen->p->iperm.p : (const int*)nullptr, bt, K_dev + (size_t)i0 * n * m);
    }
    DRE_HIP(hipGetLastError());
}
int dre_gdre_result_K_device(dre_ctx* ctx, const dre_gdre_result* r, double* K_dev) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        export_trajectory(c, r, K_dev);
        c->sync();
    });
}
int dre_gdre_result_K_all(dre_ctx* ctx, const dre_gdre_result* r, double* K_host) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const int nt = (int)r->r.Kt.size();
        if (nt == 0) return;
        const size_t tot = (size_t)nt * r->r.Kt[0].rows * r->r.Kt[0].cols;
        if (tot == 0) return;
        DevArr<double> stage(c, tot);
        export_trajectory(c, r, stage.p);
        DRE_HIP(hipMemcpyAsync(K_host, stage.p, tot * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        c->sync();
    });
}
int dre_gdre_result_X(const dre_gdre_result* r, int i, dre_ldlt** X) {
    if (r->dense || i < 0 || i >= (int)r->r.X.size()) return DRE_ERR_INVALID;
    // a final X the solve left in dense form is factored here, once, on the stream of the solve's context (gdre.hip, gdre_result_x); the
    // handle is const for the caller, the cache behind it is not
    GdreResult& res = const_cast<dre_gdre_result*>(r)->r;
    Ctx* const c = res.final_x ? res.final_x->ctx : nullptr;
    LDLtP x;
    try { x = gdre_result_x(res, i); }
    catch (const Error& e) { if (c) c->last_error = e.what(); else g_noctx_error = e.what(); return e.code; }
    catch (const std::exception& e) { if (c) c->last_error = e.what(); else g_noctx_error = e.what(); return DRE_ERR_INTERNAL; }
    auto* h = new dre_ldlt(); h->x = x; h->pen = r->pen; *X = h;
    return DRE_OK;
}
int dre_gdre_result_gale(const dre_gdre_result* r, int j, int64_t* iinfo, double* dinfo) {
    if (r->dense) return DRE_ERR_INVALID;
    if (j < 0 || j >= (int)r->r.gale.size()) return DRE_ERR_INVALID;
    const AdiResult& a = r->r.gale[j];
    iinfo[0] = a.iters; iinfo[1] = a.converged; iinfo[2] = a.warnings; iinfo[3] = a.rhs_cols;
    dinfo[0] = a.res_norm; dinfo[1] = a.abstol;
    return DRE_OK;
}
int dre_gdre_result_gale_history(const dre_gdre_result* r, int j, int64_t* counts, double* norms, int32_t* norm_iters, double* sre, double* sim) {
    if (r->dense) return DRE_ERR_INVALID;
    if (j < 0 || j >= (int)r->r.gale.size()) return DRE_ERR_INVALID;
    const AdiResult& g = r->r.gale[j];
    if (counts) { counts[0] = (int64_t)g.norms.size(); counts[1] = (int64_t)g.shifts.size(); }
    for (size_t i = 0; i < g.norms.size(); ++i) { if (norms) norms[i] = g.norms[i]; if (norm_iters) norm_iters[i] = g.norm_iters[i]; }
    for (size_t i = 0; i < g.shifts.size(); ++i) { if (sre) sre[i] = g.shifts[i].real(); if (sim) sim[i] = g.shifts[i].imag(); }
    return DRE_OK;
}
int dre_gdre_result_gales_all(const dre_gdre_result* r, int64_t* iinfo, double* dinfo, double* norms, int32_t* norm_iters, double* sre, double* sim) {
    if (r->dense) return DRE_ERR_INVALID;
    size_t on = 0, os = 0;
    for (size_t j = 0; j < r->r.gale.size(); ++j) {
        const AdiResult& g = r->r.gale[j];
        if (iinfo) {
            int64_t* ii = iinfo + 6 * j;
            ii[0] = g.iters; ii[1] = g.converged; ii[2] = g.warnings; ii[3] = g.rhs_cols; ii[4] = (int64_t)g.norms.size(); ii[5] = (int64_t)g.shifts.size();
        }
        if (dinfo) { dinfo[2 * j] = g.res_norm; dinfo[2 * j + 1] = g.abstol; }
        for (size_t i = 0; i < g.norms.size(); ++i) { if (norms) norms[on + i] = g.norms[i]; if (norm_iters) norm_iters[on + i] = g.norm_iters[i]; }
        for (size_t i = 0; i < g.shifts.size(); ++i) { if (sre) sre[os + i] = g.shifts[i].real(); if (sim) sim[os + i] = g.shifts[i].imag(); }
        on += g.norms.size(); os += g.shifts.size();
    }
    return DRE_OK;
}
int dre_gdre_result_free(dre_gdre_result* r) { delete r; return DRE_OK; }

// ---- dense path (dense_sign.hip, dense_gj.hip, dense_are.hip) ---------------------------------------------------------------------------------------------------
int dre_dense_gale_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* F, const dre_dense* R, int maxiters, double tol, int max_refine,
                         dre_dense** X, int64_t* iinfo, double* dinfo) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && F && R && X, "dre_dense_gale_solve: null argument");
        const int n = E->m.rows;
        DRE_REQUIRE(F->m.rows == n && F->m.cols == n && R->m.rows == n && R->m.cols == n, "dre_dense_gale_solve: E, F, R must be n x n");
        SignLyap lyap(c, E->m, maxiters, tol, max_refine);
        lyap.factor(F->m);
        auto* out = new dre_dense();
        out->m = Mat(c, n, n);
        SignStats s;
        try { s = lyap.solve(R->m, out->m); c->sync(); } catch (...) { delete out; throw; }
        if (iinfo) { iinfo[0] = s.iters; iinfo[1] = s.refinements; }
        if (dinfo) { dinfo[0] = s.res0; dinfo[1] = s.res; }
        *X = out;
    });
}
// a dense driver's result (single, adaptive, one member of a batch) as the handle the result accessors read; d is emptied
static dre_gdre_result* wrap_dense_result(DenseGdreResult& d, int n, int m) {
    auto* r = new dre_gdre_result();
    r->dense = true; r->n = n; r->m = m;
    r->r.t = std::move(d.t); r->r.Kt = std::move(d.Kt);
    r->Xd = std::move(d.X); r->solves = std::move(d.solves);
    return r;
}
int dre_dense_gdre_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* X0,
                         double t0, double tf, double dt, int order, int save_state, int maxiters, double tol, int max_refine,
                         dre_gdre_result** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && A && B && C && X0 && out, "dre_dense_gdre_solve: null argument");
        DenseGdreResult d = dense_gdre_solve(c, E->m, A->m, B->m, C->m, X0->m, t0, tf, dt, order, save_state != 0, maxiters, tol, max_refine);
        *out = wrap_dense_result(d, E->m.rows, B->m.cols);
    });
}
int dre_dense_gdre_solve_adaptive(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* X0,
                                  double t0, double tf, double dt0, int order, double rtol, double atol, double dt_min, double dt_max, int64_t max_steps,
                                  const double* tstops, int ntstops, int save_state, int maxiters, double tol, int max_refine, dre_gdre_result** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && A && B && C && X0 && out, "dre_dense_gdre_solve_adaptive: null argument");
        DRE_REQUIRE(ntstops >= 0 && (ntstops == 0 || tstops), "dre_dense_gdre_solve_adaptive: ntstops must be >= 0, with tstops given when it is positive");
        StepControl sc;
        sc.rtol = rtol; sc.atol = atol; sc.dt_min = dt_min; sc.dt_max = dt_max; sc.max_steps = (long)max_steps;
        sc.tstops.assign(tstops, tstops + ntstops);
        DenseAdaptiveResult d = dense_gdre_solve_adaptive(c, E->m, A->m, B->m, C->m, X0->m, t0, tf, dt0, order, sc, save_state != 0, maxiters, tol, max_refine);
        dre_gdre_result* r = wrap_dense_result(d.r, E->m.rows, B->m.cols);
        r->adaptive = true; r->accepted = d.accepted; r->rejected = d.rejected; r->step_err = std::move(d.err);
        *out = r;
    });
}
int dre_gdre_result_step_stats(const dre_gdre_result* r, int64_t* accepted_rejected, double* err) {
    if (!r || !r->adaptive) return DRE_ERR_INVALID;
    if (accepted_rejected) { accepted_rejected[0] = r->accepted; accepted_rejected[1] = r->rejected; }
    if (err) std::memcpy(err, r->step_err.data(), r->step_err.size() * sizeof(double));
    return DRE_OK;
}
int dre_dense_invert(dre_ctx* ctx, dre_dense* A, int32_t* piv, double* logabsdet) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(A, "dre_dense_invert: null argument");
        const int n = A->m.rows;
        DRE_REQUIRE(A->m.cols == n && n >= 1 && n <= DENSE_MAX_N, "dre_dense_invert: square matrix of order 1 .. " + std::to_string(DENSE_MAX_N) + " expected");
        DevArr<int> pv(c, n);
        DevArr<GjCtl> ctl(c, 1);
        DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(GjCtl), c->stream));
        gj_invert(c, A->m, pv.p, ctl.p);
        const GjCtl h = read_back(c, ctl.p);
        if (h.singular) throw Error(ERR_SINGULAR, "dre_dense_invert: singular matrix (exactly zero or non-finite pivot)");
        if (piv) { DRE_HIP(hipMemcpyAsync(piv, pv.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream)); c->sync(); }
        if (logabsdet) *logabsdet = h.logdet;
    });
}
int dre_dense_gare_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                         const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(E && A && B && Ct && X, "dre_dense_gare_solve: null argument");
        DenseGareResult r = dense_gare_solve(&ctx->c, E->m, A->m, B->m, Rinv ? &Rinv->m : nullptr, Ct->m, S ? &S->m : nullptr, maxiters, tol, max_refine);
        if (iinfo) { iinfo[0] = r.iters; iinfo[1] = r.refinements; }
        if (dinfo) { dinfo[0] = r.res0; dinfo[1] = r.res; }
        auto* out = new dre_dense();
        out->m = std::move(r.X);
        *X = out;
    });
}
int dre_dense_gare_solve_pair(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                              const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, dre_dense** Y, int64_t* iinfo, double* dinfo) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(E && A && B && Ct && X && Y, "dre_dense_gare_solve_pair: null argument");
        DenseGarePair r = dense_gare_solve_pair(&ctx->c, E->m, A->m, B->m, Rinv ? &Rinv->m : nullptr, Ct->m, S ? &S->m : nullptr, maxiters, tol, max_refine);
        if (iinfo) { iinfo[0] = r.X.iters; iinfo[1] = r.X.refinements; iinfo[2] = r.Y.iters; iinfo[3] = r.Y.refinements; }
        if (dinfo) { dinfo[0] = r.X.res0; dinfo[1] = r.X.res; dinfo[2] = r.Y.res0; dinfo[3] = r.Y.res; }
        auto Xo = std::make_unique<dre_dense>(), Yo = std::make_unique<dre_dense>();
        Xo->m = std::move(r.X.X); Yo->m = std::move(r.Y.X);
        *X = Xo.release(); *Y = Yo.release();
    });
}
int dre_dense_gare_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                            const dre_dense* S, const dre_dense* X, dre_dense** Res, double* norm) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(E && A && B && Ct && X && Res, "dre_dense_gare_residual: null argument");
        double fro = 0.0;
        Mat R = dense_gare_residual(&ctx->c, E->m, A->m, B->m, Rinv ? &Rinv->m : nullptr, Ct->m, S ? &S->m : nullptr, X->m, &fro);
        auto* out = new dre_dense();
        out->m = std::move(R);
        if (norm) *norm = fro;
        *Res = out;
    });
}
int dre_dense_stein_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* Q, int dual, int maxiters, double tol, dre_dense** X,
                          int64_t* iinfo, double* dinfo) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(E && A && Q && X, "dre_dense_stein_solve: null argument");
        DenseSteinResult r = dense_stein_solve(&ctx->c, E->m, A->m, Q->m, dual != 0, maxiters, tol);
        if (iinfo) { iinfo[0] = r.iters; iinfo[1] = 0; }
        if (dinfo) { dinfo[0] = r.step; dinfo[1] = r.step; }
        auto* out = new dre_dense();
        out->m = std::move(r.X);
        *X = out;
    });
}
int dre_dense_stein_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* Q, const dre_dense* X, int dual, dre_dense** Res,
                             double* norm, double* scaled) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(E && A && Q && X && Res, "dre_dense_stein_residual: null argument");
        Mat R = dense_stein_residual(&ctx->c, E->m, A->m, Q->m, X->m, dual != 0, norm, scaled);
        auto* out = new dre_dense();
        out->m = std::move(R);
        *Res = out;
    });
}
int dre_dense_dare_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                         const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(E && A && B && Ct && X, "dre_dense_dare_solve: null argument");
        DenseDareResult r = dense_dare_solve(&ctx->c, E->m, A->m, B->m, Rinv ? &Rinv->m : nullptr, Ct->m, S ? &S->m : nullptr, maxiters, tol, max_refine);
        if (iinfo) { iinfo[0] = r.iters; iinfo[1] = r.refinements; }
        if (dinfo) { dinfo[0] = r.res0; dinfo[1] = r.res; }
        auto* out = new dre_dense();
        out->m = std::move(r.X);
        *X = out;
    });
}
int dre_dense_dare_solve_pair(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                              const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, dre_dense** Y, int64_t* iinfo, double* dinfo) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(E && A && B && Ct && X && Y, "dre_dense_dare_solve_pair: null argument");
        DenseDarePair r = dense_dare_solve_pair(&ctx->c, E->m, A->m, B->m, Rinv ? &Rinv->m : nullptr, Ct->m, S ? &S->m : nullptr, maxiters, tol, max_refine);
        if (iinfo) { iinfo[0] = r.X.iters; iinfo[1] = r.X.refinements; iinfo[2] = r.Y.iters; iinfo[3] = r.Y.refinements; }
        if (dinfo) { dinfo[0] = r.X.res0; dinfo[1] = r.X.res; dinfo[2] = r.Y.res0; dinfo[3] = r.Y.res; }
        auto Xo = std::make_unique<dre_dense>(), Yo = std::make_unique<dre_dense>();
        Xo->m = std::move(r.X.X); Yo->m = std::move(r.Y.X);
        *X = Xo.release(); *Y = Yo.release();
    });
}
int dre_dense_dare_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                            const dre_dense* S, const dre_dense* X, dre_dense** Res, double* norm, double* scaled) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(E && A && B && Ct && X && Res, "dre_dense_dare_residual: null argument");
        Mat R = dense_dare_residual(&ctx->c, E->m, A->m, B->m, Rinv ? &Rinv->m : nullptr, Ct->m, S ? &S->m : nullptr, X->m, norm, scaled);
        auto* out = new dre_dense();
        out->m = std::move(R);
        *Res = out;
    });
}
int dre_gdre_result_X_dense(dre_ctx* ctx, const dre_gdre_result* r, int i, dre_dense** X) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(r && r->dense, "dre_gdre_result_X_dense: not a dense result");
        DRE_REQUIRE(i >= 0 && i < (int)r->Xd.size(), "state index out of range");
        Ctx* c = &ctx->c;
        auto* h = new dre_dense();
        h->m = Mat(c, r->n, r->n);
        copy_mat(c, r->Xd[(size_t)i], h->m);
        c->sync();
        *X = h;
    });
}
int dre_gdre_result_dense_stats(const dre_gdre_result* r, int64_t* iters, int64_t* refinements, double* residuals) {
    if (!r || !r->dense) return DRE_ERR_INVALID;
    for (size_t j = 0; j < r->solves.size(); ++j) {
        const SignStats& s = r->solves[j];
        if (iters) iters[j] = s.iters;
        if (refinements) refinements[j] = s.refinements;
        if (residuals) { residuals[2 * j] = s.res0; residuals[2 * j + 1] = s.res; }
    }
    return DRE_OK;
}

// ---- batched dense path (dense_batch.hip) ---------------------------------------------------------------------------------------------
// member handles -> one stack (rows x cols*batch, member b at b * rows * cols)
static Mat pack_stack(Ctx* c, int batch, const dre_dense* const* h, int rows, int cols) {
    Mat S(c, rows, cols * batch);
    for (int b = 0; b < batch; ++b) {
        Mat v = S.colsview(b * cols, cols);
        copy_mat(c, h[b]->m, v);
    }
    return S;
}
static void check_members(int batch, const dre_dense* const* h, int rows, int cols, const char* who, const char* what) {
    for (int b = 0; b < batch; ++b)
        DRE_REQUIRE(h[b] && h[b]->m.rows == rows && h[b]->m.cols == cols, std::string(who) + ": " + what + " of member " + std::to_string(b) + " must be " +
                                                                              std::to_string(rows) + " x " + std::to_string(cols));
}
static void check_batch_order(int batch, int n, const char* who) {
    DRE_REQUIRE(batch >= 1 && batch <= 65535, std::string(who) + ": batch must be in 1 .. 65535");
    DRE_REQUIRE(n >= 1 && n <= GJ_REGISTER_MAX_N, std::string(who) + ": the batched dense path inverts with the register panel, order 1 .. " +
                                                      std::to_string(GJ_REGISTER_MAX_N) + " (n = " + std::to_string(n) + ")");
}
// per-member outcomes -> status[], the context's per-member messages, dre_last_error = the first failed member's
static void report_members(dre_ctx* ctx, const std::vector<BatchMemberStatus>& st, int32_t* status) {
    ctx->batch_errors.assign(st.size(), std::string());
    bool first = true;
    for (size_t b = 0; b < st.size(); ++b) {
        if (status) status[b] = st[b].code;
        if (!st[b].code) continue;
        ctx->batch_errors[b] = st[b].msg;
        if (first) { ctx->c.last_error = st[b].msg; first = false; }
    }
}
const char* dre_batch_member_error(dre_ctx* ctx, int b) {
    if (!ctx || b < 0 || b >= (int)ctx->batch_errors.size()) return "";
    return ctx->batch_errors[(size_t)b].c_str();
}
int dre_dense_invert_batched(dre_ctx* ctx, int batch, dre_dense* const* A, int32_t* piv, double* logabsdet, int32_t* status) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(A && status && batch >= 1 && A[0], "dre_dense_invert_batched: null argument or batch < 1");
        const int n = A[0]->m.rows;
        check_batch_order(batch, n, "dre_dense_invert_batched");
        check_members(batch, A, n, n, "dre_dense_invert_batched", "A");
        const int nb = gj_batch_nb(n);
        require_memory(c, (size_t)batch * ((size_t)n * n + (size_t)2 * n * nb + n));
        Mat S = pack_stack(c, batch, A, n, n);
        Mat Pn(c, n, nb * batch), W(c, nb, n * batch);
        DevArr<int> pv(c, (size_t)n * batch);
        DevArr<BatchCtl> ctl(c, batch);
        DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(BatchCtl) * batch, c->stream));
        gj_invert_batched(c, batch, n, S.p, pv.p, ctl.p, BM_GJ, Pn.p, W.p);
        std::vector<BatchCtl> h((size_t)batch);
        DRE_HIP(hipMemcpyAsync(h.data(), ctl.p, sizeof(BatchCtl) * batch, hipMemcpyDeviceToHost, c->stream));
        if (piv) DRE_HIP(hipMemcpyAsync(piv, pv.p, (size_t)n * batch * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        c->sync();
        std::vector<BatchMemberStatus> st((size_t)batch);
        for (int b = 0; b < batch; ++b) {
            if (h[(size_t)b].s.gj.singular) {
                st[(size_t)b].code = ERR_SINGULAR;
                st[(size_t)b].msg = "dre_dense_invert_batched, member " + std::to_string(b) + ": singular matrix (exactly zero or non-finite pivot)";
                continue;
            }
            Mat v = S.colsview(b * n, n);
            copy_mat(c, v, A[b]->m);
            if (logabsdet) logabsdet[b] = h[(size_t)b].s.gj.logdet;
        }
        c->sync();
        report_members(ctx, st, status);
    });
}
// ---- frequency response (freq_response.hip) --------------------------------------------------------------------------------------------
// the two sweeps' entry points: collect the systems, run `sweep` (freq_response or transfer_eval on them), copy H, info and the members' outcomes
// out.  noun: what the K points are called in the caller's messages
static void sweep_entry(dre_ctx* ctx, const char* who, const char* noun, bool args_ok, int nsys, const dre_dense* const* E, const dre_dense* const* A,
                        const dre_dense* const* B, const dre_dense* const* C, int K, double* H_re, double* H_im, int32_t* status, int64_t* info,
                        const std::function<FreqResponse(const std::vector<FreqSystem>&)>& sweep) {
    DRE_REQUIRE(nsys >= 1, std::string(who) + ": no systems (nsys < 1)");
    DRE_REQUIRE(K >= 1, std::string(who) + ": at least one " + noun + " is needed (K >= 1)");
    DRE_REQUIRE(E && A && B && C && args_ok && H_re && H_im && status, std::string(who) + ": null argument");
    std::vector<FreqSystem> sys((size_t)nsys);
    for (int s = 0; s < nsys; ++s) {
        DRE_REQUIRE(E[s] && A[s] && B[s] && C[s], std::string(who) + ": null operand in system " + std::to_string(s));
        sys[(size_t)s] = FreqSystem{E[s]->m, A[s]->m, B[s]->m, C[s]->m};
    }
    const FreqResponse r = sweep(sys);
    std::memcpy(H_re, r.re.data(), r.re.size() * sizeof(double));
    std::memcpy(H_im, r.im.data(), r.im.size() * sizeof(double));
    if (info) { info[0] = r.chunk; info[1] = r.chunks; }
    report_members(ctx, r.status, status);
}
int dre_freq_response_batched(dre_ctx* ctx, int nsys, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                              const dre_dense* const* C, int K, const double* omega, int chunk, double* H_re, double* H_im, int32_t* status,
                              int64_t* info) {
    return guarded(ctx, [&] {
        sweep_entry(ctx, "dre_freq_response_batched", "frequency", omega != nullptr, nsys, E, A, B, C, K, H_re, H_im, status, info,
                    [&](const std::vector<FreqSystem>& sys) { return freq_response(&ctx->c, sys, std::vector<double>(omega, omega + K), chunk); });
    });
}
int dre_freq_response(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, int K, const double* omega,
                      int chunk, double* H_re, double* H_im, int32_t* status, int64_t* info) {
    return dre_freq_response_batched(ctx, 1, &E, &A, &B, &C, K, omega, chunk, H_re, H_im, status, info);
}

// ---- complex inversion and the transfer function at complex points (dense_cgj.hip, transfer_eval.hip) -----------------------------------
int dre_dense_invert_complex_batched(dre_ctx* ctx, int batch, dre_dense* const* Are, dre_dense* const* Aim, int32_t* piv, double* logabsdet,
                                     int32_t* status) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const char* who = "dre_dense_invert_complex_batched";
        DRE_REQUIRE(Are && Aim && status && batch >= 1 && Are[0], std::string(who) + ": null argument or batch < 1");
        const int n = Are[0]->m.rows;
        check_batch_order(batch, n, who);
        check_members(batch, Are, n, n, who, "Are");
        check_members(batch, Aim, n, n, who, "Aim");
        const int nb = cgj_batch_nb(n);
        require_memory(c, (size_t)batch * ((size_t)2 * n * n + (size_t)6 * n * nb + n));
        // member b: [Zr | Zi] at b * 2 n^2
        Mat S(c, n, 2 * n * batch);
        for (int b = 0; b < batch; ++b) {
            Mat vr = S.colsview(2 * b * n, n), vi = S.colsview((2 * b + 1) * n, n);
            copy_mat(c, Are[b]->m, vr);
            copy_mat(c, Aim[b]->m, vi);
        }
        Mat Pt(c, n, 2 * nb * batch), Wt(c, 2 * nb, 2 * n * batch);
        DevArr<int> pv(c, (size_t)n * batch);
        DevArr<BatchCtl> ctl(c, batch);
        DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(BatchCtl) * batch, c->stream));
        cgj_invert_batched(c, batch, n, S.p, pv.p, ctl.p, BM_GJ, Pt.p, Wt.p);
        std::vector<BatchCtl> h((size_t)batch);
        DRE_HIP(hipMemcpyAsync(h.data(), ctl.p, sizeof(BatchCtl) * batch, hipMemcpyDeviceToHost, c->stream));
        if (piv) DRE_HIP(hipMemcpyAsync(piv, pv.p, (size_t)n * batch * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        c->sync();
        std::vector<BatchMemberStatus> st((size_t)batch);
        for (int b = 0; b < batch; ++b) {
            if (h[(size_t)b].s.gj.singular) {
                st[(size_t)b].code = ERR_SINGULAR;
                st[(size_t)b].msg = std::string(who) + ", member " + std::to_string(b) + ": singular matrix (exactly zero or non-finite pivot)";
                continue;
            }
            Mat vr = S.colsview(2 * b * n, n), vi = S.colsview((2 * b + 1) * n, n);
            copy_mat(c, vr, Are[b]->m);
            copy_mat(c, vi, Aim[b]->m);
            if (logabsdet) logabsdet[b] = h[(size_t)b].s.gj.logdet;
        }
        c->sync();
        report_members(ctx, st, status);
    });
}
int dre_transfer_eval_batched(dre_ctx* ctx, int nsys, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                              const dre_dense* const* C, int K, const double* s_re, const double* s_im, int chunk, double* H_re, double* H_im,
                              int32_t* status, int64_t* info) {
    return guarded(ctx, [&] {
        sweep_entry(ctx, "dre_transfer_eval_batched", "point", s_re && s_im, nsys, E, A, B, C, K, H_re, H_im, status, info,
                    [&](const std::vector<FreqSystem>& sys) {
                        return transfer_eval(&ctx->c, sys, std::vector<double>(s_re, s_re + K), std::vector<double>(s_im, s_im + K), chunk);
                    });
    });
}
int dre_transfer_eval(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, int K, const double* s_re,
                      const double* s_im, int chunk, double* H_re, double* H_im, int32_t* status, int64_t* info) {
    return dre_transfer_eval_batched(ctx, 1, &E, &A, &B, &C, K, s_re, s_im, chunk, H_re, H_im, status, info);
}

// ---- time response: step, impulse, simulate (time_response.hip) --------------------------------------------------------------------------
int dre_time_response(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, int method, double dt, int K,
                      int kind, const double* U, int S, const double* X0, int block, double* Y, int64_t* info) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(E && A && B && C && Y, "dre_time_response: null argument");
        const TimeResponse r = time_response(&ctx->c, E->m, A->m, B->m, C->m, method, dt, K, kind, U, S, X0, block);
        std::memcpy(Y, r.Y.data(), r.Y.size() * sizeof(double));
        if (info) { info[0] = r.block; info[1] = r.blocks; info[2] = r.squarings; info[3] = r.launches; }
    });
}

int dre_dense_gale_solve_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* F, const dre_dense* const* R,
                                 int maxiters, double tol, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo, int32_t* status) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && F && R && X && status && batch >= 1 && E[0], "dre_dense_gale_solve_batched: null argument or batch < 1");
        const int n = E[0]->m.rows;
        check_batch_order(batch, n, "dre_dense_gale_solve_batched");
        check_members(batch, E, n, n, "dre_dense_gale_solve_batched", "E");
        check_members(batch, F, n, n, "dre_dense_gale_solve_batched", "F");
        check_members(batch, R, n, n, "dre_dense_gale_solve_batched", "R");
        DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, "dense path: maxiters must be in 1 .. 1000");
        require_memory(c, BatchedSignLyap::doubles_needed(batch, n, maxiters, 4));       // + the stacks of E, F, R and X
        for (int b = 0; b < batch; ++b) X[b] = nullptr;
        Mat Es = pack_stack(c, batch, E, n, n), Fs = pack_stack(c, batch, F, n, n), Rs = pack_stack(c, batch, R, n, n);
        Mat Xs(c, n, n * batch);
        BatchedSignLyap lyap(c, batch, Es, maxiters, tol, max_refine, 4);
        lyap.factor(Fs);
        std::vector<SignStats> stats;
        lyap.solve(Rs, Xs, stats);
        for (int b = 0; b < batch; ++b) {
            if (!lyap.alive(b)) continue;
            auto* out = new dre_dense();
            out->m = Mat(c, n, n);
            Mat v = Xs.colsview(b * n, n);
            copy_mat(c, v, out->m);
            X[b] = out;
            if (iinfo) { iinfo[2 * b] = stats[(size_t)b].iters; iinfo[2 * b + 1] = stats[(size_t)b].refinements; }
            if (dinfo) { dinfo[2 * b] = stats[(size_t)b].res0; dinfo[2 * b + 1] = stats[(size_t)b].res; }
        }
        c->sync();
        report_members(ctx, lyap.status(), status);
    });
}
int dre_dense_gdre_solve_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                                 const dre_dense* const* C, const dre_dense* const* X0, double t0, double tf, double dt, int order,
                                 int save_state, int maxiters, double tol, int max_refine, dre_gdre_result** out, int32_t* status) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && A && B && C && X0 && out && status && batch >= 1 && E[0] && B[0] && C[0],
                    "dre_dense_gdre_solve_batched: null argument or batch < 1");
        dense_check_order(order);
        DRE_REQUIRE(order <= 2, "dre_dense_gdre_solve_batched: only Ros1 and Ros2 (order 1, 2) are batched; order " + std::to_string(order) +
                                    " runs through dre_dense_gdre_solve");
        const int n = E[0]->m.rows, m = B[0]->m.cols, q = C[0]->m.rows;
        check_batch_order(batch, n, "dre_dense_gdre_solve_batched");
        check_members(batch, E, n, n, "dre_dense_gdre_solve_batched", "E");
        check_members(batch, A, n, n, "dre_dense_gdre_solve_batched", "A");
        check_members(batch, B, n, m, "dre_dense_gdre_solve_batched", "B");
        check_members(batch, C, q, n, "dre_dense_gdre_solve_batched", "C");
        check_members(batch, X0, n, n, "dre_dense_gdre_solve_batched", "X0");
        const int nsteps = (int)dense_time_grid(t0, tf, dt).size() - 1;
        DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, "dense path: maxiters must be in 1 .. 1000");
        require_memory(c, dense_gdre_batched_doubles(batch, n, m, q, nsteps, order, save_state != 0, maxiters));
        for (int b = 0; b < batch; ++b) out[b] = nullptr;
        Mat Es = pack_stack(c, batch, E, n, n), As = pack_stack(c, batch, A, n, n), Bs = pack_stack(c, batch, B, n, m),
            Cs = pack_stack(c, batch, C, q, n), Xs = pack_stack(c, batch, X0, n, n);
        std::vector<DenseGdreResult> res;
        std::vector<BatchMemberStatus> st;
        dense_gdre_solve_batched(c, batch, Es, As, Bs, Cs, Xs, m, q, t0, tf, dt, order, save_state != 0, maxiters, tol, max_refine, res, st);
        for (int b = 0; b < batch; ++b) out[b] = wrap_dense_result(res[(size_t)b], n, m);
        report_members(ctx, st, status);
    });
}

// dre_dense_gare_solve per member (dense_are_batch.hip).  Unlike the three calls above the return value is the first failed member's code.
int dre_dense_gare_solve_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                                 const dre_dense* const* Rinv, const dre_dense* const* Ct, const dre_dense* const* S, int maxiters, double tol,
                                 int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo, int32_t* status) {
    int first_fail = DRE_OK;
    const int rc = guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const char* who = "dre_dense_gare_solve_batched";
        DRE_REQUIRE(E && A && B && Ct && X && status && batch >= 1 && E[0] && B[0] && Ct[0], std::string(who) + ": null argument or batch < 1");
        DRE_REQUIRE(batch <= 65535, std::string(who) + ": batch must be in 1 .. 65535");
        const int n = E[0]->m.rows, m = B[0]->m.cols, q = Ct[0]->m.cols;
        DRE_REQUIRE(n >= 1 && 2 * n <= DENSE_MAX_N, std::string(who) + ": E must be square of order 1 .. " + std::to_string(DENSE_MAX_N / 2));
        check_members(batch, E, n, n, who, "E");
        check_members(batch, A, n, n, who, "A");
        check_members(batch, B, n, m, who, "B");
        check_members(batch, Ct, n, q, who, "Ct");
        // the inner matrices are optional per member: the array or single entries may be null (identity)
        bool anyR = false, anyS = false;
        for (int b = 0; b < batch; ++b) {
            if (Rinv && Rinv[b]) {
                anyR = true;
                DRE_REQUIRE(Rinv[b]->m.rows == m && Rinv[b]->m.cols == m, std::string(who) + ": Rinv of member " + std::to_string(b) + " must be m x m");
            }
            if (S && S[b]) {
                anyS = true;
                DRE_REQUIRE(S[b]->m.rows == q && S[b]->m.cols == q, std::string(who) + ": S of member " + std::to_string(b) + " must be q x q");
            }
        }
        // the batched inversion is the register panel's whatever dense_gj_panel says: gj_check_order's refusal, in its wording
        DRE_REQUIRE(2 * n <= GJ_REGISTER_MAX_N, std::string(who) + " (the Hamiltonian of order 2n): the register panel inverts matrices of order <= " +
                                                    std::to_string(GJ_REGISTER_MAX_N) + ", order = " + std::to_string(2 * n));
        DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, "dense GARE: maxiters must be in 1 .. 1000");
        DRE_REQUIRE(max_refine >= 0, "dense GARE: max_refine must be >= 0");
        require_memory(c, dense_gare_batched_doubles(batch, n, m, q, maxiters, max_refine));
        for (int b = 0; b < batch; ++b) X[b] = nullptr;
        Mat Es = pack_stack(c, batch, E, n, n), As = pack_stack(c, batch, A, n, n), Bs = pack_stack(c, batch, B, n, m),
            Cs = pack_stack(c, batch, Ct, n, q);
        auto pack_inner = [&](const dre_dense* const* h, int w) {
            Mat St(c, w, w * batch), I(c, w, w);
            set_identity(c, I);
            for (int b = 0; b < batch; ++b) {
                Mat v = St.colsview(b * w, w);
                copy_mat(c, h[b] ? h[b]->m : I, v);
            }
            return St;
        };
        Mat Rs, Ss;
        if (anyR && m > 0) Rs = pack_inner(Rinv, m);
        if (anyS && q > 0) Ss = pack_inner(S, q);
        std::vector<DenseGareResult> res;
        std::vector<BatchMemberStatus> st;
        dense_gare_solve_batched(c, batch, Es, As, Bs, Rs.p ? &Rs : nullptr, Cs, Ss.p ? &Ss : nullptr, m, q, maxiters, tol, max_refine, res, st);
        for (int b = 0; b < batch; ++b) {
            const DenseGareResult& r = res[(size_t)b];
            if (iinfo) { iinfo[2 * b] = r.iters; iinfo[2 * b + 1] = r.refinements; }
            if (dinfo) { dinfo[2 * b] = r.res0; dinfo[2 * b + 1] = r.res; }
            if (st[(size_t)b].code) {
                if (first_fail == DRE_OK) first_fail = st[(size_t)b].code;
                continue;
            }
            auto* o = new dre_dense();
            o->m = Mat(c, n, n);
            copy_mat(c, r.X, o->m);
            X[b] = o;
        }
        c->sync();
        report_members(ctx, st, status);
    });
    return rc != DRE_OK ? rc : first_fail;
}

// ---- host helpers ------------------------------------------------------------------------------
// ---- factored sign-function Lyapunov solver (dense_sign_lr.hip) -----------------------------------------------------------------------
int dre_sign_create(dre_ctx* ctx, const dre_dense* E, const dre_dense* F, int maxiters, double tol, dre_sign** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && F && out, "dre_sign_create: null argument");
        const int n = E->m.rows;
        DRE_REQUIRE(F->m.rows == n && F->m.cols == n, "dre_sign_create: E and F must be n x n");
        auto h = std::make_unique<dre_sign>();
        Mat Ec(c, n, E->m.cols);            // the handle outlives the caller's E
        copy_mat(c, E->m, Ec);
        h->s = std::make_unique<SignLyap>(c, Ec, maxiters, tol, 0, 0, true);
        h->s->factor(F->m);
        *out = h.release();
    });
}
int dre_sign_info(const dre_sign* s, int64_t* n_iters) {
    if (!s || !n_iters) return DRE_ERR_INVALID;
    *n_iters = s->s->iters();
    return DRE_OK;
}
// primal (F'XE + E'XF = -R / -G S G') and dual (F Y E' + E Y F' = ..., 109) solves on the same kept factorisation: one body per pair
static int sign_solve_lr(dre_ctx* ctx, bool dual, dre_sign* s, const dre_dense* G, const dre_dense* S, double rtol, int max_width, int max_refine,
                         dre_dense** L, dre_dense** D, int64_t* ii, double* dd, const char* null_msg) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(s && G && S && L && D, null_msg);
        auto Lo = std::make_unique<dre_dense>(), Do = std::make_unique<dre_dense>();
        const SignLrStats st = dual ? s->s->solve_lr_t(G->m, S->m, rtol, max_width, max_refine, Lo->m, Do->m)
                                    : s->s->solve_lr(G->m, S->m, rtol, max_width, max_refine, Lo->m, Do->m);
        c->sync();
        if (ii) { ii[0] = st.rank; ii[1] = st.peak_width; ii[2] = st.compressions; ii[3] = st.refinements; }
        if (dd) { dd[0] = st.res0; dd[1] = st.res; }
        *L = Lo.release(); *D = Do.release();
    });
}
static int sign_solve_dense(dre_ctx* ctx, bool dual, dre_sign* s, const dre_dense* R, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo,
                            const char* null_msg) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(s && R && X && max_refine >= 0, null_msg);
        const int n = s->s->n();
        auto out = std::make_unique<dre_dense>();
        out->m = Mat(c, n, n);
        s->s->set_max_refine(max_refine);
        const SignStats st = dual ? s->s->solve_t(R->m, out->m) : s->s->solve(R->m, out->m);
        c->sync();
        if (iinfo) { iinfo[0] = st.iters; iinfo[1] = st.refinements; }
        if (dinfo) { dinfo[0] = st.res0; dinfo[1] = st.res; }
        *X = out.release();
    });
}
int dre_sign_solve_lr(dre_ctx* ctx, dre_sign* s, const dre_dense* G, const dre_dense* S, double rtol, int max_width, int max_refine,
                      dre_dense** L, dre_dense** D, int64_t* ii, double* dd) {
    return sign_solve_lr(ctx, false, s, G, S, rtol, max_width, max_refine, L, D, ii, dd, "dre_sign_solve_lr: null argument");
}
int dre_sign_solve_dense(dre_ctx* ctx, dre_sign* s, const dre_dense* R, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo) {
    return sign_solve_dense(ctx, false, s, R, max_refine, X, iinfo, dinfo, "dre_sign_solve_dense: null argument or negative max_refine");
}
int dre_sign_solve_dense_t(dre_ctx* ctx, dre_sign* s, const dre_dense* R, int max_refine, dre_dense** Y, int64_t* iinfo, double* dinfo) {
    return sign_solve_dense(ctx, true, s, R, max_refine, Y, iinfo, dinfo, "dre_sign_solve_dense_t: null argument or negative max_refine");
}
int dre_sign_solve_lr_t(dre_ctx* ctx, dre_sign* s, const dre_dense* G, const dre_dense* S, double rtol, int max_width, int max_refine,
                        dre_dense** L, dre_dense** D, int64_t* ii, double* dd) {
    return sign_solve_lr(ctx, true, s, G, S, rtol, max_width, max_refine, L, D, ii, dd, "dre_sign_solve_lr_t: null argument");
}
int dre_sign_free(dre_ctx*, dre_sign* s) { delete s; return DRE_OK; }

// ---- dense generalized Sylvester solver (dense_sylvester.hip, 119) ---------------------------------------------------------------------
static void sylvester_info(const SylvStats& st, int64_t* iinfo, double* dinfo) {
    if (iinfo) { iinfo[0] = st.iters; iinfo[1] = st.refinements; }
    if (dinfo) { dinfo[0] = st.res0; dinfo[1] = st.res; dinfo[2] = st.step; }
}
int dre_dense_sylvester_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* F, const dre_dense* B, const dre_dense* C,
                              int transposed, int maxiters, double tol, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(A && B && C && X, "dre_dense_sylvester_solve: null argument");
        DenseSylvesterResult r = dense_sylvester_solve(&ctx->c, E ? &E->m : nullptr, A->m, F ? &F->m : nullptr, B->m, C->m, transposed != 0, maxiters, tol,
                                                       max_refine);
        sylvester_info(r.st, iinfo, dinfo);
        auto* out = new dre_dense();
        out->m = std::move(r.X);
        *X = out;
    });
}
int dre_dense_sylvester_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* F, const dre_dense* B, const dre_dense* C,
                                 const dre_dense* X, int transposed, dre_dense** Res, double* norm, double* scaled) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(A && B && C && X && Res, "dre_dense_sylvester_residual: null argument");
        Mat R = dense_sylvester_residual(&ctx->c, E ? &E->m : nullptr, A->m, F ? &F->m : nullptr, B->m, C->m, X->m, transposed != 0, norm, scaled);
        auto* out = new dre_dense();
        out->m = std::move(R);
        *Res = out;
    });
}
int dre_sylvester_create(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* F, const dre_dense* B, int maxiters, double tol,
                         dre_sylvester** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(A && B && out, "dre_sylvester_create: null argument");
        const int n = A->m.rows, m = B->m.rows;
        DRE_REQUIRE(n >= 1 && m >= 1 && A->m.cols == n && B->m.cols == m && (!E || (E->m.rows == n && E->m.cols == n)) &&
                        (!F || (F->m.rows == m && F->m.cols == m)),
                    "dre_sylvester_create: E and A must be n x n, F and B m x m");
        DRE_REQUIRE(n <= DENSE_MAX_N && m <= DENSE_MAX_N, "dre_sylvester_create: orders of at most " + std::to_string(DENSE_MAX_N) + " expected");
        auto h = std::make_unique<dre_sylvester>();
        Mat Ec(c, n, n), Fc(c, m, m);            // the handle outlives the caller's E and F
        if (E) copy_mat(c, E->m, Ec); else set_identity(c, Ec);
        if (F) copy_mat(c, F->m, Fc); else set_identity(c, Fc);
        h->s = std::make_unique<SignSylvester>(c, Ec, Fc, maxiters, tol, 0);
        h->s->factor(A->m, B->m);
        *out = h.release();
    });
}
int dre_sylvester_solve(dre_ctx* ctx, dre_sylvester* s, const dre_dense* C, int transposed, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(s && C && X && max_refine >= 0, "dre_sylvester_solve: null argument or negative max_refine");
        auto out = std::make_unique<dre_dense>();
        out->m = Mat(c, s->s->n(), s->s->m());
        s->s->set_max_refine(max_refine);
        const SylvStats st = transposed ? s->s->solve_t(C->m, out->m) : s->s->solve(C->m, out->m);
        c->sync();
        sylvester_info(st, iinfo, dinfo);
        *X = out.release();
    });
}
int dre_sylvester_iters(const dre_sylvester* s, int64_t* n_iters) {
    if (!s || !n_iters) return DRE_ERR_INVALID;
    *n_iters = s->s->iters();
    return DRE_OK;
}
int dre_sylvester_destroy(dre_ctx*, dre_sylvester* s) { delete s; return DRE_OK; }

// device SVD and balanced truncation (110)
int dre_svd_jacobi(dre_ctx* ctx, const dre_dense* A, double tol, dre_dense** U, dre_dense** S, dre_dense** V, int64_t* stats) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(A && U && S && V, "dre_svd_jacobi: null argument");
        SvjStats st;
        SvdResult r = svd_jacobi(c, A->m, tol, &st);
        c->sync();
        auto Uo = std::make_unique<dre_dense>(), So = std::make_unique<dre_dense>(), Vo = std::make_unique<dre_dense>();
        Uo->m = r.U; So->m = r.S; Vo->m = r.V;
        if (stats) { stats[0] = st.sweeps; stats[1] = st.rounds; stats[2] = st.rank; }
        *U = Uo.release(); *S = So.release(); *V = Vo.release();
    });
}
int dre_balance_lr(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* Lc, const dre_dense* Dc,
                   const dre_dense* Lo, const dre_dense* Do, int order, double tol, dre_dense** hsv, dre_dense** T, dre_dense** W, dre_dense** Ar,
                   dre_dense** Br, dre_dense** Cr, int64_t* ii, double* dd) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && A && B && C && Lc && Dc && Lo && Do && hsv && T && W && Ar && Br && Cr, "dre_balance_lr: null argument");
        BalanceResult r = balance_lr(c, E->m, A->m, B->m, C->m, Lc->m, Dc->m, Lo->m, Do->m, order, tol);
        c->sync();
        std::unique_ptr<dre_dense> o[6];
        const Mat* src[6] = {&r.hsv, &r.T, &r.W, &r.Ar, &r.Br, &r.Cr};
        for (int i = 0; i < 6; ++i) { o[i] = std::make_unique<dre_dense>(); o[i]->m = *src[i]; }
        if (ii) { ii[0] = r.order; ii[1] = r.rank; ii[2] = r.r_c; ii[3] = r.r_o; ii[4] = r.dropped; ii[5] = r.sweeps; }
        if (dd) { dd[0] = r.eye_err; dd[1] = r.bound; dd[2] = r.neg_max; }
        *hsv = o[0].release(); *T = o[1].release(); *W = o[2].release(); *Ar = o[3].release(); *Br = o[4].release(); *Cr = o[5].release();
    });
}
// LQG balanced truncation from the two Riccati solutions (113)
int dre_lqg_balance(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* X, const dre_dense* Y,
                    int order, double tol, dre_dense** mu, dre_dense** T, dre_dense** W, dre_dense** Ar, dre_dense** Br, dre_dense** Cr, dre_dense** Kr,
                    dre_dense** Lr, dre_dense** Ac, int64_t* ii, double* dd) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && A && B && C && X && Y && mu && T && W && Ar && Br && Cr && Kr && Lr && Ac, "dre_lqg_balance: null argument");
        LqgBalanceResult l = lqg_balance(c, E->m, A->m, B->m, C->m, X->m, Y->m, order, tol);
        const BalanceResult& r = l.bal;
        c->sync();
        std::unique_ptr<dre_dense> o[9];
        const Mat* src[9] = {&r.hsv, &r.T, &r.W, &r.Ar, &r.Br, &r.Cr, &l.Kr, &l.Lr, &l.Ac};
        for (int i = 0; i < 9; ++i) { o[i] = std::make_unique<dre_dense>(); o[i]->m = *src[i]; }
        if (ii) { ii[0] = r.order; ii[1] = r.rank; ii[2] = r.r_c; ii[3] = r.r_o; ii[4] = r.dropped; ii[5] = r.sweeps; }
        if (dd) { dd[0] = r.eye_err; dd[1] = r.bound; dd[2] = r.neg_max; }
        dre_dense** dst[9] = {mu, T, W, Ar, Br, Cr, Kr, Lr, Ac};
        for (int i = 0; i < 9; ++i) *dst[i] = o[i].release();
    });
}

// batched block Jacobi and ensemble balanced truncation (111)
static std::vector<Mat> member_mats(int batch, const dre_dense* const* h, const char* who, const char* what) {
    std::vector<Mat> v((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        DRE_REQUIRE(h[b], std::string(who) + ": " + what + " of member " + std::to_string(b) + " is null");
        v[(size_t)b] = h[b]->m;
    }
    return v;
}
int dre_sym_eig_jacobi_batched(dre_ctx* ctx, int batch, const dre_dense* const* S, double tol, dre_dense** values, dre_dense** vectors, int64_t* stats,
                               int32_t* status) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const char* who = "dre_sym_eig_jacobi_batched";
        DRE_REQUIRE(S && values && vectors && status && batch >= 1, std::string(who) + ": null argument or batch < 1");
        for (int b = 0; b < batch; ++b) values[b] = vectors[b] = nullptr;
        SymEigBatch r = sym_eig_jacobi_batch(c, member_mats(batch, S, who, "S"), tol, who);
        // ascending order and the output format of dre_sym_eig_jacobi, per member; the eigenvalues of all members go up in one copy
        const int q = r.eig[0].q;
        std::vector<double> w((size_t)batch * q);
        DevArr<double> dw(c, w.size());
        std::vector<std::unique_ptr<dre_dense>> Vo((size_t)batch), Wo((size_t)batch);
        for (int b = 0; b < batch; ++b) {
            if (r.status[(size_t)b].code) continue;
            const SymEig& e = r.eig[(size_t)b];
            std::vector<int> ids(e.j);
            for (int i = 0; i < e.j; ++i) ids[i] = i;
            std::sort(ids.begin(), ids.end(), [&](int a, int d) { return e.w[a] < e.w[d]; });
            for (int i = 0; i < e.j; ++i) w[(size_t)b * q + i] = e.w[ids[i]];
            Vo[(size_t)b] = std::make_unique<dre_dense>();
            Vo[(size_t)b]->m = sym_eig_backtransform(c, e, ids);
        }
        dw.upload(c, w);
        for (int b = 0; b < batch; ++b) {
            if (r.status[(size_t)b].code) continue;
            Wo[(size_t)b] = std::make_unique<dre_dense>();
            Wo[(size_t)b]->m.buf = dw.buf; Wo[(size_t)b]->m.p = dw.p + (size_t)b * q;
            Wo[(size_t)b]->m.rows = q; Wo[(size_t)b]->m.cols = 1; Wo[(size_t)b]->m.ld = q > 0 ? q : 1;
            if (stats) { stats[2 * b] = r.stats[(size_t)b].sweeps; stats[2 * b + 1] = r.stats[(size_t)b].rounds; }
        }
        c->sync();
        for (int b = 0; b < batch; ++b) { values[b] = Wo[(size_t)b].release(); vectors[b] = Vo[(size_t)b].release(); }
        report_members(ctx, r.status, status);
    });
}
int dre_svd_jacobi_batched(dre_ctx* ctx, int batch, const dre_dense* const* A, double tol, dre_dense** U, dre_dense** S, dre_dense** V, int64_t* stats,
                           int32_t* status) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const char* who = "dre_svd_jacobi_batched";
        DRE_REQUIRE(A && U && S && V && status && batch >= 1, std::string(who) + ": null argument or batch < 1");
        for (int b = 0; b < batch; ++b) U[b] = S[b] = V[b] = nullptr;
        SvdBatch r = svd_jacobi_batch(c, member_mats(batch, A, who, "A"), tol, who);
        c->sync();
        std::vector<std::unique_ptr<dre_dense>> o((size_t)3 * batch);
        for (int b = 0; b < batch; ++b) {
            if (r.status[(size_t)b].code) continue;
            const Mat* src[3] = {&r.svd[(size_t)b].U, &r.svd[(size_t)b].S, &r.svd[(size_t)b].V};
            for (int i = 0; i < 3; ++i) { o[(size_t)3 * b + i] = std::make_unique<dre_dense>(); o[(size_t)3 * b + i]->m = *src[i]; }
            if (stats) { stats[3 * b] = r.stats[(size_t)b].sweeps; stats[3 * b + 1] = r.stats[(size_t)b].rounds; stats[3 * b + 2] = r.stats[(size_t)b].rank; }
        }
        for (int b = 0; b < batch; ++b) { U[b] = o[(size_t)3 * b].release(); S[b] = o[(size_t)3 * b + 1].release(); V[b] = o[(size_t)3 * b + 2].release(); }
        report_members(ctx, r.status, status);
    });
}
int dre_balance_lr_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                           const dre_dense* const* C, const dre_dense* const* Lc, const dre_dense* const* Dc, const dre_dense* const* Lo,
                           const dre_dense* const* Do, int order, double tol, dre_dense** hsv, dre_dense** T, dre_dense** W, dre_dense** Ar,
                           dre_dense** Br, dre_dense** Cr, int64_t* ii, double* dd, int32_t* status) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const char* who = "dre_balance_lr_batched";
        DRE_REQUIRE(E && A && B && C && Lc && Dc && Lo && Do && hsv && T && W && Ar && Br && Cr && status && batch >= 1,
                    std::string(who) + ": null argument or batch < 1");
        dre_dense** outs[6] = {hsv, T, W, Ar, Br, Cr};
        for (int b = 0; b < batch; ++b)
            for (auto* o : outs) o[b] = nullptr;
        const dre_dense* const* ins[8] = {E, A, B, C, Lc, Dc, Lo, Do};
        std::vector<BalanceMember> mem((size_t)batch);
        for (int b = 0; b < batch; ++b) {
            for (auto* in : ins) DRE_REQUIRE(in[b], std::string(who) + ": a handle of member " + std::to_string(b) + " is null");
            mem[(size_t)b] = BalanceMember{&E[b]->m, &A[b]->m, &B[b]->m, &C[b]->m, &Lc[b]->m, &Dc[b]->m, &Lo[b]->m, &Do[b]->m};
        }
        BalanceBatch r = balance_lr_batch(c, mem, order, tol, who);
        c->sync();
        std::vector<std::unique_ptr<dre_dense>> o((size_t)6 * batch);
        for (int b = 0; b < batch; ++b) {
            if (r.status[(size_t)b].code) continue;
            const BalanceResult& m = r.res[(size_t)b];
            const Mat* src[6] = {&m.hsv, &m.T, &m.W, &m.Ar, &m.Br, &m.Cr};
            for (int i = 0; i < 6; ++i) { o[(size_t)6 * b + i] = std::make_unique<dre_dense>(); o[(size_t)6 * b + i]->m = *src[i]; }
            if (ii) { int64_t* p = ii + 6 * (size_t)b; p[0] = m.order; p[1] = m.rank; p[2] = m.r_c; p[3] = m.r_o; p[4] = m.dropped; p[5] = m.sweeps; }
            if (dd) { double* p = dd + 3 * (size_t)b; p[0] = m.eye_err; p[1] = m.bound; p[2] = m.neg_max; }
        }
        for (int b = 0; b < batch; ++b)
            for (int i = 0; i < 6; ++i) outs[i][b] = o[(size_t)6 * b + i].release();
        report_members(ctx, r.status, status);
    });
}

int dre_host_eigvals(int n, const double* A, double* wr, double* wi) {
    return guarded(nullptr, [&] {
        std::vector<double> M(A, A + (size_t)n * n);
        auto ev = host_eigvals(n, M);
        for (int i = 0; i < n; ++i) { wr[i] = ev[i].real(); wi[i] = ev[i].imag(); }
    });
}
int dre_host_gen_eigvals(int n, const double* A, const double* E, double* wr, double* wi) {
    return guarded(nullptr, [&] {
        std::vector<double> Av(A, A + (size_t)n * n), Ev(E, E + (size_t)n * n);
        auto ev = host_gen_eigvals(n, Av, Ev);
        for (int i = 0; i < n; ++i) { wr[i] = ev[i].real(); wi[i] = ev[i].imag(); }
    });
}
int dre_host_svd_left(int p, int w, const double* R, double* U, double* sv) {
    return guarded(nullptr, [&] {
        std::vector<double> Rv(R, R + (size_t)p * w), Uv, s;
        host_svd_left(p, w, Rv, Uv, s);
        std::memcpy(U, Uv.data(), Uv.size() * sizeof(double));
        std::memcpy(sv, s.data(), s.size() * sizeof(double));
    });
}

}  // extern "C"
