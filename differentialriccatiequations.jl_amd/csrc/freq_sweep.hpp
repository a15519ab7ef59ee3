// The chunked sweep that freq_response.hip and transfer_eval.hip share (internal): K points of one or several systems
// of one (n, m, q), member s K + k = system s at point k, as many members per chunk as the plan of freq_chunk.hpp allows.  Everything the two
// methods have in common is here: the validation of the operands, the chunk plan and its ERR_ALLOC, the result, the chunk loop with its split
// at system boundaries, the read-backs and the per-member status.  A method describes itself by a struct (no base class; the driver is a
// template over it):
//   name, noun, nouns, sym, pencil    the words of the messages: "freq_response", "frequency", "frequencies", "omega", "i omega E - A"
//   points() / points_msg             K (0: invalid) and the message for that; finite(k); point_text(k) for a failed member's message
//   order_msg(n)                      empty, or why the order is beyond the method's register panel
//   panel_ok(n) / panel_fn            the panel width of freq_chunk.hpp against the inversion's own table, and that table's name
//   member_doubles(n, m, q), fixed_doubles(K)      the device memory of one member and of the points
//   allocate(ctx, n, m, q, cs)        the points on the device and a chunk's workspace (the control blocks and H are the driver's)
//   assemble(ctx, f, b0, cnt, k0)     the matrices of members [b0, b0 + cnt) of the chunk: system f at points k0 ..
//   invert(ctx, len, ctl)             the chunk's inversion in place
//   solve(ctx, f, b0, cnt, k0, ctl, Hre, Him)      Y, its refinement step and Re H, Im H of those members
#pragma once
#include <cmath>

#include "freq_response.hpp"
#include "profiling.hpp"

namespace dre {

inline size_t free_doubles(Ctx* ctx) {                   // what require_memory compares with
    size_t fr = 0, total = 0;
    DRE_HIP(hipMemGetInfo(&fr, &total));
    return (fr + ctx->pool.cached_bytes()) / sizeof(double);
}

template <class Method>
FreqResponse freq_sweep(Ctx* ctx, const std::vector<FreqSystem>& sys, int chunk, Method& md) {
    const std::string who = std::string(Method::name) + ": ";
    DRE_REQUIRE(!sys.empty(), who + "no systems");
    const size_t points = md.points();
    DRE_REQUIRE(points > 0, who + Method::points_msg);
    DRE_REQUIRE(points <= 2147483647u, who + "too many " + Method::nouns);
    for (size_t k = 0; k < points; ++k) DRE_REQUIRE(md.finite(k), who + Method::noun + " " + std::to_string(k) + " is not finite");
    const int n = sys[0].E.rows, m = sys[0].B.cols, q = sys[0].C.rows;
    DRE_REQUIRE(n >= 1 && m >= 1 && q >= 1, who + "n, m and q must be at least 1");
    for (size_t s = 0; s < sys.size(); ++s) {
        const FreqSystem& f = sys[s];
        DRE_REQUIRE(f.E.rows == n && f.E.cols == n && f.A.rows == n && f.A.cols == n && f.B.rows == n && f.B.cols == m && f.C.rows == q && f.C.cols == n,
                    who + "system " + std::to_string(s) + ": E and A must be " + std::to_string(n) + " x " + std::to_string(n) + ", B " +
                        std::to_string(n) + " x " + std::to_string(m) + " and C " + std::to_string(q) + " x " + std::to_string(n));
    }
    const std::string order = md.order_msg(n);
    DRE_REQUIRE(order.empty(), who + order);
    DRE_REQUIRE(chunk >= 0 && chunk <= FR_MAX_CHUNK, who + "chunk must be in 0 .. 65535 (0: as many members as fit)");
    const int K = (int)points;
    DRE_REQUIRE(md.panel_ok(n), who + "panel width table out of step with " + Method::panel_fn);
    const long long members = (long long)sys.size() * K;
    const size_t qm = (size_t)q * m;
    DRE_REQUIRE((unsigned long long)members * qm <= (1ull << 40), who + "result too large");

    // the plan, and the memory of a whole chunk (and the points) before the first kernel
    const size_t avail = free_doubles(ctx), fixed = md.fixed_doubles(K), per = md.member_doubles(n, m, q);
    const FrChunkPlan plan = fr_chunk_plan_of(avail > fixed ? avail - fixed : 0, per, members, chunk);
    if (plan.err == FR_PLAN_MEMORY)
        throw Error(ERR_ALLOC, who + (chunk > 0 ? "a chunk of " + std::to_string(std::min<long long>(chunk, members)) + " members" : std::string("one member")) +
                                   " needs " + std::to_string(((size_t)std::max<long long>(1, std::min<long long>(chunk, members)) * per * 8) >> 20) +
                                   " MiB of device memory, " + std::to_string((avail * 8) >> 20) + " MiB available");
    DRE_REQUIRE(plan.err == FR_PLAN_OK, who + "invalid chunk plan");
    DRE_REQUIRE(plan.chunks <= 2147483647LL, who + "too many chunks");
    const int cs = plan.chunk;
    require_memory(ctx, (size_t)cs * per + fixed);

    FreqResponse out;
    out.chunk = cs; out.chunks = (int)plan.chunks;
    out.re.assign((size_t)members * qm, 0.0);
    out.im.assign((size_t)members * qm, 0.0);
    out.status.assign((size_t)members, BatchMemberStatus{});

    md.allocate(ctx, n, m, q, cs);
    DevArr<double> H(ctx, 2 * qm * cs);
    DevArr<BatchCtl> ctl(ctx, (size_t)cs);
    std::vector<BatchCtl> hctl((size_t)cs);
    std::vector<double> hH(2 * qm * cs);
    const double nan = std::nan("");

    for (long long g0 = 0; g0 < members; g0 += cs) {
        const int len = (int)std::min<long long>(cs, members - g0);
        double* Hre = H.p;
        double* Him = H.p + (size_t)len * qm;
        DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(BatchCtl) * (size_t)len, ctx->stream));
        // the members of one system that fall into this chunk share that system's operands: [b0, b1) of the chunk, points k0 ..
        auto segments = [&](auto&& f) {
            for (int b0 = 0; b0 < len;) {
                const long long g = g0 + b0;
                const int s = (int)(g / K), k0 = (int)(g % K), b1 = (int)std::min<long long>(len, b0 + (K - k0));
                f(sys[(size_t)s], b0, b1 - b0, k0);
                b0 = b1;
            }
        };
        segments([&](const FreqSystem& f, int b0, int cnt, int k0) { md.assemble(ctx, f, b0, cnt, k0); });
        DRE_HIP(hipGetLastError());
        md.invert(ctx, len, ctl.p);
        segments([&](const FreqSystem& f, int b0, int cnt, int k0) { md.solve(ctx, f, b0, cnt, k0, ctl.p, Hre, Him); });
        DRE_HIP(hipGetLastError());
        // one copy of the chunk's Re H and Im H, one of its control blocks
        DRE_HIP(hipMemcpyAsync(hH.data(), H.p, sizeof(double) * 2 * qm * (size_t)len, hipMemcpyDeviceToHost, ctx->stream));
        DRE_HIP(hipMemcpyAsync(hctl.data(), ctl.p, sizeof(BatchCtl) * (size_t)len, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        for (int b = 0; b < len; ++b) {
            const size_t g = (size_t)(g0 + b), s = g / (size_t)K, k = g % (size_t)K;
            double* re = out.re.data() + g * qm;
            double* im = out.im.data() + g * qm;
            if (hctl[(size_t)b].s.gj.singular) {
                BatchMemberStatus& st = out.status[g];
                st.code = ERR_SINGULAR;
                st.msg = std::string(Method::name) + ", system " + std::to_string(s) + ", " + Method::noun + " " + std::to_string(k) + " (" + Method::sym + " = " +
                         md.point_text(k) + "): " + Method::pencil + " is singular (exactly zero or non-finite pivot: " + Method::sym +
                         " on a pole, or a non-finite entry)";
                for (size_t t = 0; t < qm; ++t) { re[t] = nan; im[t] = nan; }
                continue;
            }
            std::memcpy(re, hH.data() + (size_t)b * qm, sizeof(double) * qm);
            std::memcpy(im, hH.data() + ((size_t)len + b) * qm, sizeof(double) * qm);
        }
    }
    return out;
}

}  // namespace dre
