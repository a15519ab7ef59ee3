// Host decisions of the low-rank ADI (engine.hip), free of HIP so that a stand-alone host program can test them (tests/test_adi_plan_host.py):
// the partial-fraction coefficients of a fan group, which shifts a group takes, which rank owns which solve and where its columns live in
// the gathered panel, the list of distinct real shifts that still need something, and the ledger of the iterations a chunk enqueued
// speculatively with its replay against the iteration count the device reports.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstring>
#include <vector>

namespace dre {

#define FAN_GMAX 10
struct FanCoef { double c[FAN_GMAX][FAN_GMAX], d[FAN_GMAX][FAN_GMAX]; };
struct FanSlots { int s[FAN_GMAX]; };       // solve s lives in columns s[s] k .. of the panel (shift-sharded groups: slab of the owning rank)

// c_js and d_js of the fan groups (engine.hip, "Fan groups") for the g real shifts mu[0..g); returns max_j sum_s |c_js|
inline double fan_coefficients(const double* mu, int g, FanCoef* out) {
    long double c[FAN_GMAX][FAN_GMAX] = {{0}}, d[FAN_GMAX][FAN_GMAX] = {{0}};
    double worst = 0.0;
    for (int j = 0; j < g; ++j) {
        long double sum = 0.0L;
        for (int s = 0; s <= j; ++s) {
            long double num = 1.0L, den = 1.0L;
            for (int i = 0; i < j; ++i) num *= -(long double)mu[s] - (long double)mu[i];
            for (int i = 0; i <= j; ++i) if (i != s) den *= (long double)mu[i] - (long double)mu[s];
            c[j][s] = num / den;
            sum += fabsl(c[j][s]);
        }
        worst = std::max(worst, (double)sum);
    }
    for (int j = 0; j < g; ++j)
        for (int s = 0; s <= j; ++s) {
            long double acc = 0.0L;
            for (int i = s; i <= j; ++i) acc += 2.0L * (long double)mu[i] * c[i][s];
            d[j][s] = acc;
        }
    for (int j = 0; j < FAN_GMAX; ++j) for (int s = 0; s < FAN_GMAX; ++s) { out->c[j][s] = (double)c[j][s]; out->d[j][s] = (double)d[j][s]; }
    return worst;
}

// The shifts of the next fan group: the leading real shifts of `ups` up to the first repeated value, at most `room` (<= FAN_GMAX), cut back
// while the coefficient sum exceeds max_coef.  Returns g with mus[0..g) and *co filled (also for g = 1), or 0 where fewer than gmin remain.
inline int fan_pick(const std::vector<std::complex<double>>& ups, int room, int gmin, double max_coef, double* mus, FanCoef* co) {
    int g = 0;
    while (g < (int)ups.size() && g < room && ups[(size_t)g].imag() == 0.0) {
        bool dup = false;
        for (int i = 0; i < g; ++i) dup = dup || mus[i] == ups[(size_t)g].real();
        if (dup) break;
        mus[g] = ups[(size_t)g].real(); ++g;
    }
    while (g >= 2 && fan_coefficients(mus, g, co) > max_coef) --g;
    if (g == 1) (void)fan_coefficients(mus, 1, co);
    if (g < gmin) g = 0;
    return g;
}

// Who solves what in a group of g shifts on P ranks.  Ownership goes by the shift's position in the LIST (pos0 = position of the group's first
// shift, list_size = 0: no list, the group position counts), not in the group: the same shift always meets the same rank.  A group that wraps
// around the end of the list may give one rank more than g / P solves: gp is the largest share, W_s lives in slab owner[s] of the gathered
// panel (gp solves wide), in the owner's order.
struct FanLayout {
    int owner[FAN_GMAX];
    int gp = 0;
    FanSlots slots;
    std::vector<std::vector<int>> pos;       // per rank: its group positions, ascending
};
inline FanLayout fan_layout(int g, int P, size_t pos0, size_t list_size) {
    FanLayout L;
    std::memset(L.owner, 0, sizeof(L.owner));
    std::memset(&L.slots, 0, sizeof(L.slots));
    L.pos.resize((size_t)P);
    for (int s = 0; s < g; ++s) {
        const int o = (int)((list_size ? (pos0 + (size_t)s) % list_size : (size_t)s) % (size_t)P);
        L.owner[s] = o;
        L.pos[(size_t)o].push_back(s);
        L.gp = std::max(L.gp, (int)L.pos[(size_t)o].size());
    }
    for (int r = 0; r < P; ++r)
        for (size_t z = 0; z < L.pos[(size_t)r].size(); ++z) L.slots.s[L.pos[(size_t)r][z]] = r * L.gp + (int)z;
    return L;
}

// The distinct real values of a shift list that `reject(position in the list, value)` does not turn down, in list order, at most `cap`.
// Complex shifts are passed over; the predicate is asked once per real value that is not in the result yet, while there is room.
template <typename Reject>
std::vector<double> distinct_real_shifts(const std::vector<std::complex<double>>& values, size_t cap, Reject reject) {
    std::vector<double> out;
    for (size_t i = 0; i < values.size() && out.size() < cap; ++i) {
        if (values[i].imag() != 0.0) continue;
        const double v = values[i].real();
        if (std::find(out.begin(), out.end(), v) != out.end()) continue;
        if (!reject(i, v)) out.push_back(v);
    }
    return out;
}

// What a chunk enqueued speculatively, one record per iteration (a conjugate pair is one record of two shifts and is never split), and the
// replay once the device has reported how many iterations it accepted.
template <typename Payload>
struct ChunkLedger {
    struct Rec { int iters_after; size_t nblocks; int nshifts; Payload payload; };
    struct Replay {
        size_t nblocks;                  // block count of the iterate after the last accepted record (the chunk's start: none accepted)
        int nshifts = 0;                 // accepted shifts
        const Payload* last = nullptr;   // payload of the last accepted record; nullptr: the chunk start
        std::vector<int> accepted;       // iters_after of the accepted records, in order
    };
    size_t blocks_before = 0;
    std::vector<Rec> recs;
    bool empty() const { return recs.empty(); }
    size_t size() const { return recs.size(); }
    void add(int iters_after, size_t nblocks, int nshifts, const Payload& payload) { recs.push_back({iters_after, nblocks, nshifts, payload}); }
    Replay replay(int h_iters) const {
        Replay rp;
        rp.nblocks = blocks_before;
        for (auto& r : recs) {
            if (r.iters_after <= h_iters) {
                rp.nblocks = r.nblocks; rp.nshifts += r.nshifts;
                rp.last = &r.payload;
                rp.accepted.push_back(r.iters_after);
            }
        }
        return rp;
    }
};

}  // namespace dre
