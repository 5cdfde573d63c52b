// svg-ir_amd/csrc/workload_history.hpp -- the speculation history of the forward (api.hip): what recent views of each workload needed.
// Host code only (no HIP): tests/test_workload_history.py compiles it into a small host program and checks its rules.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <mutex>

namespace svgir {

// A workload.  (P is NOT part of a workload's identity as long as it moves slowly: densification / pruning changes it every few hundred iterations,
// scene/gaussian_model.py:1229-1253, and the history must survive that -- every sample remembers the Gaussian count it was taken at and
// is scaled to the caller's: instances and state slots grow with the surfel count on a fixed view.  A caller whose P is more than a
// factor of two away from the entry's latest sample is another model: it gets its own entry, and a scaled sample never exceeds four
// times the largest unscaled one.  `scope` = svgir_params.workload_scope: models that share (device, image size, widths, variant) keep
// separate histories by giving each its own id.)
struct CapKey { int dev, W, H, P, S, VS, variant, scope; };

// Speculative-capacity history: the instance counts of the last eight forwards PER WORKLOAD KEY, so that scenes / resolutions that
// alternate in one process (a 256x256 preview next to a 1600x1600 render, several scenes, several devices) neither re-run each other's
// dependent stages nor over-allocate each other's blobs.  A small fixed table, least-recently-used replacement.  Thread-safe.
class WorkloadHistory {
public:
    // Depth-key speculation.  The depth keys are positive floats; in a bounded scene they share their top byte (sign + 7 exponent bits: all
    // depths in [2, 8), or [8, 32) ...), and then the fourth 8-bit pass of the depth sort orders nothing.  The preprocess reports AND / OR
    // of the visible keys' top bytes (read back with the instance count); once kTopStreak consecutive views of a workload had one common
    // byte, the next view is launched with three passes, its culled keys carrying that byte -- and re-run from scratch, with four, if a
    // visible key turns out to differ (the streak then starts over, so at most one view in kTopStreak + 1 can ever be re-run).
    static constexpr int kTopStreak = 3;
    static constexpr int kEntries = 16;
    // speculation counters (svgir_speculation_stats): forwards, re-runs for the instance capacity, for the state-slot capacity, for the
    // depth-key byte, views sorted in three passes
    enum Stat { kForwards, kRerunR, kRerunSlots, kRerunTop, kThreePass, kStats };

    // the largest instance count (0: none seen) and *slots the largest state-slot total (common.hpp seg_slots summed over the sub-tiles;
    // -1: none seen) of the workload's recent views, scaled to k.P
    int guess(const CapKey& k, long long* slots) {
        std::lock_guard<std::mutex> lk(mu_);
        const Entry* e = find(k, false);
        long long m = 0, raw = 0, ms = -1, raws = 0;
        if (e) for (unsigned i = 0; i < std::min(e->next, 8u); i++) { m = std::max(m, scale_to(e->hist[i], e->hist_P[i], k.P)); raw = std::max<long long>(raw, e->hist[i]); }
        if (e && e->next_slots) for (unsigned i = 0; i < std::min(e->next_slots, 8u); i++) { ms = std::max(ms, scale_to(e->hist_slots[i], e->hist_slots_P[i], k.P)); raws = std::max(raws, e->hist_slots[i]); }
        *slots = ms < 0 ? ms : std::min(ms, 4 * raws + 64);
        return (int)std::min<long long>(std::min(m, 4 * raw), 0x7ffff000LL);
    }
    void record_R(const CapKey& k, int R) {
        std::lock_guard<std::mutex> lk(mu_);
        Entry* e = find(k, true);
        e->hist[e->next % 8] = R; e->hist_P[e->next % 8] = k.P;
        e->next++;
        e->key.P = k.P;   // (the entry follows its model's Gaussian count)
    }
    void record_slots(const CapKey& k, long long slots, long long nonempty) {
        std::lock_guard<std::mutex> lk(mu_);
        Entry* e = find(k, true);
        e->hist_slots[e->next_slots % 8] = slots; e->hist_slots_P[e->next_slots % 8] = k.P;
        e->next_slots++;
        if (nonempty >= 0) { e->fill = nonempty + 1; e->fill_P = k.P; }   // (stored + 1: a zero-initialised entry has seen none)
    }
    // The FILL of the composite launch: non-empty sub-tiles (= waves with work) of the workload's latest view.  The forward composite exists
    // in two occupancy variants (render_fwd.hip): below ~4 rounds of waves the machine is under-filled and the variant with more registers
    // per wave wins; above, the one with more resident waves.  -1: no view seen yet.
    long long guess_fill(const CapKey& k) {
        std::lock_guard<std::mutex> lk(mu_);
        const Entry* e = find(k, false);
        return (e && e->fill > 0) ? e->fill - 1 : -1;
    }
    // the common top byte to speculate on, or -1
    int guess_top(const CapKey& k) {
        std::lock_guard<std::mutex> lk(mu_);
        const Entry* e = find(k, false);
        return (e && e->top_streak >= kTopStreak) ? e->top_byte : -1;
    }
    void record_top(const CapKey& k, uint32_t summary) {   // {AND << 8 | OR}; AND = 0xff, OR = 0: nothing visible (no information)
        const int av = (int)((summary >> 8) & 0xffu), ov = (int)(summary & 0xffu);
        if (av == 0xff && ov == 0) return;
        std::lock_guard<std::mutex> lk(mu_);
        Entry* e = find(k, true);
        if (av != ov) { e->top_streak = 0; return; }
        if (e->top_streak > 0 && e->top_byte == av) e->top_streak = std::min(e->top_streak + 1, 1 << 20);
        else { e->top_byte = av; e->top_streak = 1; }
    }
    // image blob of the workload's latest forward (its slot total is read when the next one starts) and its Gaussian count; null: none
    const void* last_view(const CapKey& k, int* P) {
        std::lock_guard<std::mutex> lk(mu_);
        const Entry* e = find(k, false);
        if (e) *P = e->last_view_P;
        return e ? e->last_view : nullptr;
    }
    void set_last_view(const CapKey& k, const void* image_blob, int P) {
        std::lock_guard<std::mutex> lk(mu_);
        Entry* e = find(k, true);
        e->last_view = image_blob; e->last_view_P = P;
    }
    // forgets the workloads of one scope (all of them: scope < 0)
    void reset(int scope) {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto& e : table_)
            if (e.used && (scope < 0 || e.key.scope == scope)) e = Entry{};
    }
    void count(Stat s) { stats_[s]++; }
    void stats(int64_t* out) const { for (int i = 0; i < kStats; i++) out[i] = (int64_t)stats_[i].load(); }

private:
    struct Entry { CapKey key; int hist[8]; int hist_P[8]; long long hist_slots[8]; int hist_slots_P[8]; unsigned next, next_slots; unsigned long long stamp; bool used;
                   long long fill; int fill_P;   // non-empty 8x8 sub-tiles of the workload's latest view (-1 / 0: none seen), and its Gaussian count
                   int top_byte, top_streak;   // common top byte of the visible depth keys of the last `top_streak` views (0: none / not common)
                   const void* last_view; int last_view_P; };
    static bool same_key(const CapKey& a, const CapKey& b) {   // a: the entry's key (P = the Gaussian count of its latest sample), b: the caller's
        if (!(a.dev == b.dev && a.W == b.W && a.H == b.H && a.S == b.S && a.VS == b.VS && a.variant == b.variant && a.scope == b.scope)) return false;
        return a.P <= 0 || b.P <= 0 || ((long long)a.P <= 2ll * b.P && (long long)b.P <= 2ll * a.P);
    }
    static long long scale_to(long long v, int from_P, int to_P) {   // a count measured at from_P Gaussians, expected at to_P
        if (from_P <= 0 || from_P == to_P) return v;
        return (long long)((double)v * (double)to_P / (double)from_P) + 1;
    }
    // the first matching entry (its use refreshed), else with `create` the least recently used one, emptied; mu_ held
    Entry* find(const CapKey& k, bool create) {
        Entry* lru = &table_[0];
        for (auto& e : table_) {
            if (e.used && same_key(e.key, k)) { e.stamp = ++clock_; return &e; }
            if (!e.used) { if (lru->used) lru = &e; }
            else if (lru->used && e.stamp < lru->stamp) lru = &e;
        }
        if (!create) return nullptr;
        *lru = Entry{};
        lru->key = k; lru->used = true; lru->stamp = ++clock_;
        return lru;
    }

    std::mutex mu_;
    Entry table_[kEntries] = {};
    unsigned long long clock_ = 0;
    std::atomic<long long> stats_[kStats] = {};
};

}  // namespace svgir
