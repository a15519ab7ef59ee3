// C ABI of libdre_hip (declared in include/dre_hip.h), core: version, context, options, profiler, dense handles, pencil, the GEMM / SpMM / QR /
// symmetric eigensolver entries and the host helpers.  The families live beside it: api_lowrank.hip (shift solves, LDLt, ADI, communicator,
// GDRE), api_dense.hip (the dense solvers), api_probe.hip (the test and diagnostic surface); abi.hpp holds what they share.
#include "abi.hpp"

#include <algorithm>
#include <cstring>
#include <functional>

#include "comm.hpp"
#include "hostla.hpp"
#include "sym_jacobi.hpp"

using namespace dre;

thread_local std::string dre::g_noctx_error;

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
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        DRE_REQUIRE(rows >= 0 && cols >= 0 && ld >= std::max(rows, 1), "dre_dense_upload: bad shape");
        dre_dense* d = put(o, out, Mat(&ctx->c, rows, cols));
        if (rows > 0 && cols > 0) {
            DRE_HIP(hipMemcpy2DAsync(d->m.p, (size_t)d->m.ld * sizeof(double), host, (size_t)ld * sizeof(double),
                                     (size_t)rows * sizeof(double), cols, hipMemcpyHostToDevice, ctx->c.stream));
            DRE_HIP(hipStreamSynchronize(ctx->c.stream));
        }
    });
}
int dre_dense_create(dre_ctx* ctx, int rows, int cols, dre_dense** out) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        DRE_REQUIRE(rows >= 0 && cols >= 0, "dre_dense_create: bad shape");
        fill_mat(&ctx->c, put(o, out, Mat(&ctx->c, rows, cols))->m, 0.0);
    });
}
int dre_dense_download(dre_ctx* ctx, const dre_dense* a, double* host, int ld) {
    return guarded(ctx, [&] { download_mat(&ctx->c, a->m, host, ld); });
}
// device-to-device interop with buffers the caller owns (e.g. the exchange tensors handed to RCCL): column-major, leading dimension ld
int dre_dense_from_device(dre_ctx* ctx, int rows, int cols, const double* src_dev, int ld, dre_dense** out) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        DRE_REQUIRE(rows >= 0 && cols >= 0 && ld >= std::max(rows, 1), "dre_dense_from_device: bad shape");
        dre_dense* d = put(o, out, Mat(&ctx->c, rows, cols));
        if (rows > 0 && cols > 0)
            DRE_HIP(hipMemcpy2DAsync(d->m.p, (size_t)d->m.ld * sizeof(double), src_dev, (size_t)ld * sizeof(double), (size_t)rows * sizeof(double), cols,
                                     hipMemcpyDeviceToDevice, ctx->c.stream));
        DRE_HIP(hipStreamSynchronize(ctx->c.stream));
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
    return guarded_out<dre_pencil>(ctx, [&](AbiOut<dre_pencil>& o) {
        dre_pencil* h = o.make(out);
        h->p = pencil_create(ctx ? &ctx->c : nullptr, n, Ep, Ei, Ev, Ap, Ai, Av, base, leaf, upload, &h->hE, &h->hA);
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

// ---- kernels -----------------------------------------------------------------------------------
int dre_gemm(dre_ctx* ctx, int tA, int tB, double alpha, const dre_dense* A, const dre_dense* B, double beta, dre_dense* C) {
    return guarded(ctx, [&] { gemm(&ctx->c, tA != 0, tB != 0, alpha, A->m, B->m, beta, C->m); });
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
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        Mat A(c, L->m.rows, L->m.cols);
        copy_mat(c, L->m, A);
        QRFact f = qr_factor(c, A);
        dre_dense* Q = put(o, Qo, Mat(c, f.m, f.kq));
        set_identity(c, Q->m, 1.0);
        qr_apply_q(c, f, Q->m, false);
        put(o, Ro, f.R);
    });
}
// the result of either symmetric eigensolver as the entries return it: eigenvalues ascending in a column, their vectors in that order
static void eig_out(Ctx* c, const SymEig& e, DenseOut& o, dre_dense** values, dre_dense** vectors) {
    std::vector<int> ids(e.j);
    for (int i = 0; i < e.j; ++i) ids[i] = i;
    std::sort(ids.begin(), ids.end(), [&](int a, int b) { return e.w[a] < e.w[b]; });
    std::vector<double> w(e.j);
    for (int i = 0; i < e.j; ++i) w[i] = e.w[ids[i]];
    put(o, vectors, sym_eig_backtransform(c, e, ids));
    dre_dense* W = put(o, values, Mat(c, e.j, 1));
    if (e.j) {
        DRE_HIP(hipMemcpyAsync(W->m.p, w.data(), e.j * sizeof(double), hipMemcpyHostToDevice, c->stream));
        DRE_HIP(hipStreamSynchronize(c->stream));
    }
}
int dre_sym_eig(dre_ctx* ctx, const dre_dense* S, double tolfac, dre_dense** values, dre_dense** vectors) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        Mat A(c, S->m.rows, S->m.cols);
        copy_mat(c, S->m, A);
        // (this entry IS the Householder + QL solver, whatever sym_eig_method says; the Jacobi solver has dre_sym_eig_jacobi)
        struct Method0 { Ctx* c; int was; ~Method0() { c->sym_eig_method = was; } } method0{c, c->sym_eig_method};
        c->sym_eig_method = 0;
        SymEig e = sym_eig(c, A, tolfac > 0 ? tolfac : 4.0);
        eig_out(c, e, o, values, vectors);
    });
}
int dre_sym_eig_jacobi(dre_ctx* ctx, const dre_dense* S, double tol, dre_dense** values, dre_dense** vectors, int64_t* stats) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(S && values && vectors, "dre_sym_eig_jacobi: null argument");
        BjStats bs;
        SymEig e = sym_eig_jacobi(c, S->m, tol, &bs);
        eig_out(c, e, o, values, vectors);
        if (stats) { stats[0] = bs.sweeps; stats[1] = bs.rounds; }
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
