// svg-ir_amd/csrc/render_bwd_plain.hip -- backward alpha compositing at the widths WITHOUT vfeatures (rgss, and svgss
// with VS = 0): replaces the backward renderCUDA of rgss backward.cu:431-757 (svgss backward.cu:529-934 with VS = 0).
//
// Same decomposition as render_bwd.hip (one wave64 per 64-candidate depth segment of an 8x8 sub-tile, started from the
// forward's dumped blend state), but built around how a gfx950 SIMD issues instructions (scripts/probes/valu_rate_probe.hip,
// measured): ONE wave issues one VALU instruction per ~8 cycles whether or not the instructions depend on each other, and a
// SIMD only reaches its 2 cycles per wave64 instruction with >= 4-6 resident waves.  So instruction-level parallelism inside
// a wave buys nothing, registers spent on it cost resident waves, and every instruction counts.  Hence:
//   * one candidate at a time (no lock-step groups); 10 112 B of LDS per wave keep 16 waves per CU (4 per SIMD, pinned by
//     amdgpu_waves_per_eu) resident, which leaves each lane 128 VGPRs -- 102 to 119 are used, no scratch;
//   * the per-candidate attributes are wave-uniform.  The records of a block of 8 candidates (float4 #0 .. #4 of each: 640 B)
//     are copied global -> LDS by the DMA path (global_load_lds, no VGPRs), and phase A reads candidate k's values back with
//     broadcast ds_read_b128 (every lane the same address) into VGPRs, which enter the per-pixel math as operands.  LDS
//     returns in order, so the record of the next candidate is in flight behind a COUNTED lgkmcnt wait while this one is
//     evaluated; no scalar memory load is left inside the candidate loop (scalar loads return out of order: every wait on one
//     is lgkmcnt(0), and a record that misses the scalar cache had one candidate's work to arrive in -- DESIGN.md 4,
//     profiles/bwd_lds_records_ab.txt).  ONE record buffer: the copy for block n + 1 is issued in phase B of block n, behind
//     the last read of the buffer and in front of the moment MFMAs, and is waited for (vmcnt(0)) behind those MFMAs, in
//     front of the block's first atomics;
//   * all per-Gaussian sums over the 64 pixels run on the matrix pipe.  The blend weight w and ONE more per-(pixel,
//     candidate) scalar v = G dL_dalpha go to an LDS panel (8 candidates per block); the w rows of TWO consecutive blocks x
//     G[pixel][colour3 normal3 depth feature S] give the channel gradients of 16 candidates in one 16-row contraction (3 MFMAs per
//     candidate in all, not 4), rows v x Mom[pixel][1 px py px^2 px py py^2] give per block six pixel moments from
//     which the six geometric gradients (mean2D.xy, conic.xyz, opacity) follow per candidate:
//         sum_p v dx = X M0 - M1,  sum_p v dx^2 = X (X M0 - 2 M1) + M3,  ...   (X, Y, px, py relative to the sub-tile centre)
//     with dL_ddist = v (-0.5 opacity) -- v_mfma_f32_16x16x4_f32, exact fp32 products;
//   * the un-weighted depth-differencing term (quirk Q5) needs sum_p [pixel blends] (-gD): one DPP wave reduction per candidate;
//   * results: float atomics into ONE packed gradient row per Gaussian (common.hpp packed_row_geom), unpacked by geom_bwd.hip.
#include <algorithm>

#include "common.hpp"
#include "stage.hpp"
#include "dev_trace.hpp"

namespace svgir {

namespace {

#ifndef BWDP_GRID_MULT
#define BWDP_GRID_MULT 4   // workgroups launched per resident wave slot
#endif
#ifndef BWDP_WPE
#define BWDP_WPE 4
#endif
#ifndef BWDP_MFMA_ACC
#define BWDP_MFMA_ACC 1   // accumulators per 16-long MFMA chain (2: even and odd steps apart, summed at the end -- profiles/bwd_rows_ab.txt)
#endif
#ifndef BWDP_AHEAD
#define BWDP_AHEAD 1      // phase A reads the record of candidate k + BWDP_AHEAD from LDS while it evaluates candidate k (profiles/bwd_lds_records_ab.txt)
#endif
#ifndef BWDP_HOIST
#define BWDP_HOIST 0      // 1: let the compiler keep the moment operands and lane-derived addresses in VGPRs across blocks (profiles/bwd_lds_records_ab.txt)
#endif
#if BWDP_HOIST
#define BWDP_OPAQUE(x) ((void)0)
#else
#define BWDP_OPAQUE(x) asm volatile("" : "+v"(x))   // the value is re-derived behind this point, not carried in registers across it
#endif

template <int S>
struct PlainGeom {
    static constexpr int SB = 8;                 // candidates per panel (8 w rows + 8 v rows)
    static constexpr int NC0 = 7 + S;            // colour3, normal3, depth, feature S
    static constexpr int GROW = NC0 + 1;
    static constexpr int PS = 68;                // panel row stride (floats)
    static constexpr int PROWS = 32;             // panel rows: 2 x 8 blend weights w (a PAIR of blocks) | 8 v | 8 u (Q5 term) of the current block
    static constexpr size_t off_m = (size_t)PROWS * PS * 4;            // moments + Q5 sums [SB][8]
    static constexpr int NCH = 5;                // record float4 #0 .. #4 of a candidate: everything phase A and the epilogue read
    static constexpr size_t off_c = off_m + (size_t)SB * 8 * 4;        // the block's records [NCH][SB] float4 (LDS-DMA target)
    static constexpr size_t off_q = off_c + (size_t)NCH * SB * 16;     // the segment's {gid, slot} entries, deepest first
    static constexpr size_t lds_bytes = off_q + (size_t)SEG * 8;
    static_assert(NC0 <= 16, "one 16-wide MFMA column tile");
    static_assert((size_t)64 * GROW * 4 <= off_m, "the G transposition tile aliases the panel");
    static_assert(S == 0 || rec_embeds_features(S, 0), "phase A reads the feature row out of the staged record");
    static_assert(lds_bytes <= 10240, "16 waves per CU (4 per SIMD) must stay resident: 160 KB of LDS");
};

template <int S, bool SVGSS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BWDP_WPE, BWDP_WPE)))
render_bwd_plain_kernel(const RenderBwdArgs a) {
    using PG = PlainGeom<S>;
    constexpr int SB = PG::SB, NC0 = PG::NC0, GROW = PG::GROW, PS = PG::PS;
    constexpr int SS = S > 0 ? S : 1;
    constexpr int GEO = packed_row_geom(S).GEO, RS = packed_row_geom(S).RS;   // common.hpp: the packed row of a Gaussian
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sP = reinterpret_cast<float*>(smem);                    // [32][PS] rows 0..15: blend weights of two blocks, 16..23: v, 24..31: u
    float* sG = sP;                                                // [64][GROW] upstream gradients (transposition only)
    float* sM = reinterpret_cast<float*>(smem + PG::off_m);        // [SB][8] six moments, Q5 sum, pad
    float4* sC = reinterpret_cast<float4*>(smem + PG::off_c);      // [NCH][SB] record float4 #0 .. #4 of the block's candidates
    uint2* sQ = reinterpret_cast<uint2*>(smem + PG::off_q);        // [SEG] {gid, slot}, deepest first

    const int lane = threadIdx.x;
    const bool surface = cfg_flag(a.cfg, 0), normalize_depth = cfg_flag(a.cfg, 1);
    const bool sp = surface && cfg_flag(a.cfg, 2);
    const bool bgeom = SVGSS ? true : (a.backward_geometry != 0);
    const size_t N_ = (size_t)a.W * a.H;
    const float ddelx_dx = 0.5f * a.W, ddely_dy = 0.5f * a.H;
    const int colB = lane & 15, grpB = lane >> 4;

    // B operand of the moment contraction, lane l: Mom[pixel 16 (l >> 4) + kk][column l & 15] = X(mx(kk & 7)) Y(my(kk >> 3)),
    // (mx, my) = pixel position inside the 8x8 sub-tile minus 3.5, columns 1, px, py, px^2, px py, py^2 (others 0):
    // X(m) = cx0 + m (cx1 + m cx2) with one-hot (cx0, cx1, cx2) by column -- evaluated between the MFMAs, where the wave
    // waits for the matrix pipe anyway -- and Y for the lane's two pixel rows in momy[2]
    float cx0, cx1, cx2, momy[2];
    {
        const int ex = colB == 1 || colB == 4 ? 1 : colB == 3 ? 2 : 0;
        const int ey = colB == 2 || colB == 4 ? 1 : colB == 5 ? 2 : 0;
        cx0 = (colB < 6 && ex == 0) ? 1.f : 0.f; cx1 = ex == 1 ? 1.f : 0.f; cx2 = ex == 2 ? 1.f : 0.f;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const float my = (float)(2 * grpB + h) - 3.5f;
            momy[h] = ey == 0 ? 1.f : ey == 1 ? my : my * my;
        }
    }

    typedef const __attribute__((address_space(4))) uint32_t cu32;
    // the segment count and this wave's first descriptor are independent loads (the list position of a work id does not
    // depend on the count: common.hpp seg_item_of)
    cu32* dsc0 = (cu32*)(uintptr_t)(a.seg_desc + min(seg_item_of(blockIdx.x), (uint32_t)a.seg_cap));
    uint32_t d_sm = dsc0[0], d_r0 = dsc0[1], d_len = dsc0[2], d_count = dsc0[3], d_ndump = dsc0[4], d_sb = dsc0[6];
    // The caller's gradient tensors start from zero and are first touched by the kernels BEHIND this one: every wave of the grid clears
    // its share here -- stores the wave never waits for, in a kernel that is bound by latency, not by bandwidth -- instead of a memset
    // on a side stream that has to be forked from and joined with the caller's stream.
    if (a.clear) {
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        for (size_t i = (size_t)blockIdx.x * 64 + threadIdx.x; i < a.clear_n16; i += (size_t)gridDim.x * 64) a.clear[i] = z;
    }
    const uint32_t nlive = min(a.seg_count[0], (uint32_t)a.seg_cap);
    const uint32_t nwork = seg_work_ids(nlive);
    if (blockIdx.x >= nwork) return;
    DEV_TRACE_DECL();
    [[maybe_unused]] unsigned dev_items = 0, dev_cands = 0;
    for (uint32_t w = blockIdx.x; w < nwork; w += gridDim.x) {
    // longest-first list, dealt to the XCDs in blocks of consecutive items
    const uint32_t item = seg_item_of(w);
    if (item >= nlive) continue;
    if (w != blockIdx.x) {
        cu32* dsc = (cu32*)(uintptr_t)(a.seg_desc + item);
        d_sm = dsc[0]; d_r0 = dsc[1]; d_len = dsc[2]; d_count = dsc[3]; d_ndump = dsc[4]; d_sb = dsc[6];
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): no LDS-DMA of the previous segment lands once this one's set-up has begun
    wave_lds_sync();   // the previous segment's LDS traffic is complete before its buffers are reused
    const uint32_t sm = d_sm, r0 = d_r0, tlen = d_len;
    const int count = (int)d_count, ndump = (int)d_ndump;
    const int sid = (int)(sm >> SEG_K_BITS), kseg = (int)(sm & ((1u << SEG_K_BITS) - 1u));
    const int tile = sid >> 2, sub = sid & 3;
    const int seg_lo = kseg * SEG, seg_hi = min(count, seg_lo + SEG);
    if (seg_hi <= seg_lo) continue;
    const int tx = tile % a.gx, ty = tile / a.gx;
    const int px = tx * TILE + (sub & 1) * 8 + (lane & 7);
    const int py = ty * TILE + (sub >> 1) * 8 + (lane >> 3);
    const bool inside = px < a.W && py < a.H;
    const float pxf = (float)px, pyf = (float)py;
    const float cxs = (float)(tx * TILE + (sub & 1) * 8) + 3.5f, cys = (float)(ty * TILE + (sub >> 1) * 8) + 3.5f;   // sub-tile centre
    const uint2* __restrict__ sub_in = a.sub_list + (size_t)4 * r0 + (size_t)sub * tlen;
    const size_t pid = inside ? (size_t)a.W * py + px : 0;
    const int nent = seg_hi - seg_lo;
    // the segment's list entries, deepest first: loaded here, stored to sQ behind the per-pixel loads
    uint2 ent_in = make_uint2(0u, 0u);
    if (lane < nent) ent_in = sub_in[seg_hi - 1 - lane];

    // Per-candidate attributes (wave-uniform).  The block's records lie in LDS (sC, copied there by the DMA path); candidate k's
    // values come from broadcast ds_read_b128 -- every lane reads the same address -- and its slot from the sQ entry.  They stay in
    // VGPRs and enter the per-pixel arithmetic as operands.  LDS returns in order, so the waits are counted: the record of
    // candidate k + BWDP_AHEAD is in flight while candidate k is evaluated, and no scalar memory load is left inside the loop.
    struct Cand { float X, Y, cxx, cxy, cyy, op, dep, DA, DB, cr, cg, cb, nx, ny, nz, f[SS]; uint32_t slot; };
    auto read_cand = [&](int c0, int k) -> Cand {
        const float4 q0 = sC[k], q1 = sC[SB + k], q3 = sC[3 * SB + k], q4 = sC[4 * SB + k];
        Cand c;
        c.X = q0.x; c.Y = q0.y; c.cxx = q0.z; c.cxy = q0.w; c.cyy = q1.x; c.op = q1.y; c.dep = q1.z; c.DA = q1.w;
        c.DB = q3.x; c.cr = q3.y; c.cg = q3.z; c.cb = q3.w; c.nx = q4.x; c.ny = q4.y; c.nz = q4.z;
        if (S > 0) {   // the feature row rides in the record (preprocess; common.hpp rec_feature_slot: float4 #2, then R_IU)
            const float4 q2 = sC[2 * SB + k];
            const float fv[5] = {q2.x, q2.y, q2.z, q2.w, q4.w};
#pragma unroll
            for (int ch = 0; ch < SS; ch++) c.f[ch] = fv[ch];
        } else {
            c.f[0] = 0.f;
        }
        // (uniform select) slots beyond the list replay the record of the list's last entry and never blend: slot 2^32-1,
        // whatever the staged record and the sQ entry hold
        const uint32_t sl = sQ[c0 + k].y;
        c.slot = c0 + k < nent ? sl : 0xffffffffu;
        return c;
    };

    const float T_final = inside ? a.final_T[pid] : 0.f;
    const float D_final = (inside && normalize_depth) ? a.final_D[pid] : 0.f;
    const uint32_t last_contributor = inside ? (uint32_t)a.n_contrib[pid] : 0u;
    float gC[3], gN[3], gF[SS], gD = 0.f, gO = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++) { gC[i] = (inside && a.g_color) ? a.g_color[i * N_ + pid] : 0.f; gN[i] = (inside && a.g_normal) ? a.g_normal[i * N_ + pid] : 0.f; }
#pragma unroll
    for (int i = 0; i < SS; i++) gF[i] = (inside && i < S && a.g_feature) ? a.g_feature[i * N_ + pid] : 0.f;
    if (inside) { gD = a.g_depth ? a.g_depth[pid] : 0.f; gO = a.g_opacity ? a.g_opacity[pid] : 0.f; }
    const float bgdot = a.bg[0] * gC[0] + a.bg[1] * gC[1] + a.bg[2] * gC[2];
    const float omt = 1.f - T_final;
    const float gDn = normalize_depth ? gD / omt : gD;  // depth gradient seen by the blended depth
    // d(depth normalisation)/d alpha of the reference, gD*D_final/(1-Tf)^2 * -Tf/(1-alpha)/T_new, equals kdn / T_old
    const float kdn = normalize_depth ? -gD * D_final * T_final / (omt * omt) : 0.f;
    const float gO_kbg = gO - (bgdot + (normalize_depth ? 0.f : 10.f * gD));   // opacity minus background (+ un-normalised depth) term
    const float q5g = sp ? -gD : 0.f;   // Q5: un-weighted depth-differencing term

    // deepest contributor of the wave
    uint32_t wmax = last_contributor;
    wmax = wave_reduce_max(wmax);
    if (wmax == 0) continue;

    // Replay state: the per-channel recurrences of the reference collapse into ONE scalar recurrence on
    // A = sum_ch accum_ch g_ch with s = sum_ch value_ch g_ch (render_bwd.hip):  A <- last_alpha s_last + (1 - last_alpha) A ;
    // dL_dalpha += s - A.
    float T = T_final;
    float last_alpha = 0.f;
    float A_acc = 0.f, s_last = 0.f;
    if (kseg < ndump) {
        // Not the deepest live segment: start from the forward state dumped at this segment's far end.  With
        // last_alpha = 0 the recurrence takes accum = blend of everything behind = (final - prefix) / T_end.
        constexpr int NST = 8 + S;
        const uint32_t sbase = d_sb;   // state slot of (sub-tile, 0)
        const float* e = a.seg_state + ((size_t)(sbase + kseg) * NST) * 64 + lane;
        const float* f = a.seg_state + ((size_t)(sbase + ndump) * NST) * 64 + lane;   // final state
        T = e[0];
        float dot = (f[7 * 64] - e[7 * 64]) * gDn;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            dot += (f[(1 + i) * 64] - e[(1 + i) * 64]) * gC[i];
            dot += (f[(4 + i) * 64] - e[(4 + i) * 64]) * gN[i];   // zero unless `surface` (the forward leaves N at 0)
        }
        if (bgeom) {
#pragma unroll
            for (int i = 0; i < S; i++) dot += (f[(8 + i) * 64] - e[(8 + i) * 64]) * gF[i];
        }
        A_acc = dot * __builtin_amdgcn_rcpf(T);
    }

    // G matrix of this sub-tile, row = pixel (lane), columns = [colour3 | normal3 x10 (Q4) | depth | feature S]; phase B needs
    // it as the MFMA B operand (lane l: G[pixel 16 (l >> 4) + kk][channel l & 15], kk = 0..15): transposed once through LDS
    {
        float* g = sG + lane * GROW;
        g[0] = gC[0]; g[1] = gC[1]; g[2] = gC[2];
        g[3] = surface ? gN[0] * 10.f : 0.f; g[4] = surface ? gN[1] * 10.f : 0.f; g[5] = surface ? gN[2] * 10.f : 0.f;
        g[6] = gDn;
#pragma unroll
        for (int i = 0; i < S; i++) g[7 + i] = gF[i];
    }
    float Bp[16];
    wave_lds_sync();
    {
        const float* gB = sG + (16 * grpB) * GROW + (colB < NC0 ? colB : 0);
#pragma unroll
        for (int kk = 0; kk < 16; kk++) Bp[kk] = colB < NC0 ? gB[kk * GROW] : 0.f;
    }
    wave_lds_sync();   // sG aliases the panel
    // (the weight rows of a pair's second block enter the channel contraction also where that block never runs -- masked there, finite here)
#pragma unroll
    for (int k = 0; k < SB; k++) sP[(SB + k) * PS + lane] = 0.f;

    // The segment's list entries, deepest first (the replay walks back to front): gid for the DMA sources and the atomics of
    // phase B, slot for phase A
    int nskip = 0;   // entries that lie behind every pixel of this wave (a prefix: slots descend)
    sQ[lane] = ent_in;
    nskip = __popcll(__ballot(lane < nent && ent_in.y >= wmax));
    // flags folded into the per-pixel factors: the replay itself is branch-free
    const float gNe0 = surface ? gN[0] : 0.f, gNe1 = surface ? gN[1] : 0.f, gNe2 = surface ? gN[2] : 0.f;
    float gFe[SS];
#pragma unroll
    for (int i = 0; i < SS; i++) gFe[i] = bgeom ? gF[i] : 0.f;
    const float spf = sp ? 1.f : 0.f;
    const float gOT = gO_kbg * T_final;

    const int cstart = (nskip / SB) * SB;   // (uniform) the deepest entries lie behind every pixel of the wave: start further in
    // The records of a block (lane = (float4 of the record, candidate)): copied global -> LDS by the DMA path, no VGPRs.  ONE buffer:
    // the copy for block n + 1 is issued once block n has read its last value out of it (phase B below), here for the first block.
    // Slots beyond the list take the record of the list's last entry.  32-bit offsets: P * 96 B < 4 GiB (api.hip validate)
    auto stage_records = [&](int cb) {
        int lC = lane;
        BWDP_OPAQUE(lC);
        if (lC < PG::NCH * SB) {
            const int cq = lC & 7, chunk = lC >> 3;
            const uint32_t gq = sQ[min(cb + cq, nent - 1)].x;
            const float* src = a.rec + (uint32_t)(gq * (uint32_t)REC + (uint32_t)(4 * chunk));
            __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(smem + PG::off_c), 16, 0, 0);
        }
    };
    wave_lds_sync();   // sQ visible
    stage_records(cstart);
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): the first block's records have landed
    wave_lds_sync();
    DEV_TRACE_MARK(0);   // segment setup
    dev_items++; dev_cands += (unsigned)nent;
    // Blocks are taken in PAIRS counted from cstart: the blend weights of both blocks fill the 16 rows of ONE channel contraction
    // (w_a | w_b) x G behind the pair's second block -- or behind the segment's last block, then with the rows of the block that did
    // not run masked.  Moments and geometric gradients stay per block.
    uint32_t live16 = 0;   // live bits of the pair: first block in bits 0..7, second in 8..15 (wave-uniform)
    for (int c0 = cstart; c0 < nent; c0 += SB) {
        const int par = ((c0 - cstart) / SB) & 1;   // (uniform) position of the block in its pair
        float* sPw = sP + par * (SB * PS) + lane;   // this block's weight rows
        uint32_t live = 0;  // bit k set: candidate c0+k has at least one blending pixel (wave-uniform)
        const bool more = c0 + SB < nent;           // (uniform) another block follows: its records are staged from phase B
        // ---------------- phase A: lane = pixel, one candidate at a time, attributes broadcast from LDS into VGPRs ----------------
        // (LDS reads and stores retire in order: the panel stores of candidate k are issued behind the reads of candidate
        // k + BWDP_AHEAD, and every wait is a counted one)
        float hw = 0.f, hv = 0.f, hu = 0.f;
        Cand cand[SB];
#pragma unroll
        for (int k = 0; k < BWDP_AHEAD; k++) cand[k] = read_cand(c0, k);
#pragma unroll
        for (int k = 0; k < SB; k++) {
            if (k + BWDP_AHEAD < SB) cand[k + BWDP_AHEAD] = read_cand(c0, k + BWDP_AHEAD);
            const Cand& cur = cand[k];
            const float dx = cur.X - pxf, dy = cur.Y - pyf;
            if (k > 0) {
                sPw[(k - 1) * PS] = hw; sP[(2 * SB + k - 1) * PS + lane] = hv; sP[(3 * SB + k - 1) * PS + lane] = hu;
            }
            const float pw = pair_power(cur.cxx, cur.cxy, cur.cyy, dx, dy);
            const float Gs = exp_nonpos(pw);
            const float al = fminf(0.99f, cur.op * Gs);
            const bool pre = cur.slot < last_contributor && pw <= 0.0f && al >= (1.0f / 255.0f);
            const float oma = 1.f - al;
            const float ioma = __builtin_amdgcn_rcpf(oma);
            // (a b + c d has two fused forms; which one is written out, so that the sums do not depend on where the compiler finds the
            // operands -- the forms are those of the scalar-operand build this path was measured against, profiles/bwd_lds_records_ab.txt)
            float sd = __builtin_fmaf(cur.cb, gC[2], __builtin_fmaf(cur.cr, gC[0], cur.cg * gC[1]));
            sd += __builtin_fmaf(cur.nz, gNe2, __builtin_fmaf(cur.ny, gNe1, cur.nx * gNe0));
            const float d_cur = cur.dep - spf * __builtin_fmaf(dy, cur.DB, dx * cur.DA);   // depth differencing (common.hpp R_DA / R_DB)
            sd += d_cur * gDn;
#pragma unroll
            for (int ch = 0; ch < S; ch++) sd += cur.f[ch] * gFe[ch];
            // the sequential part: T <- T / (1 - alpha) and the scalar replay recurrence (backward.cu:700-850)
            const float inv_Told = __builtin_amdgcn_rcpf(T);
            // T / (1 - alpha) to half an ulp: product with the rounded reciprocal plus one residual step (render_bwd.hip)
            const float Tq = T * ioma;
            const float Tn = __builtin_fmaf(__builtin_fmaf(-oma, Tq, T), ioma, Tq);
            const float An = last_alpha * s_last + (1.f - last_alpha) * A_acc;
            float dL_dalpha = kdn * inv_Told + (sd - An);
            dL_dalpha *= Tn;
            dL_dalpha += gOT * ioma;
            T = pre ? Tn : T;
            A_acc = pre ? An : A_acc;
            s_last = pre ? sd : s_last;
            last_alpha = pre ? al : last_alpha;
            hw = pre ? al * Tn : 0.f;              // blend weight
            hv = pre ? Gs * dL_dalpha : 0.f;       // v
            hu = pre ? q5g : 0.f;                  // u: its pixel sum is the Q5 term (0 unless per-pixel depth is on)
            live |= (__builtin_amdgcn_ballot_w64(pre) != 0ull ? 1u : 0u) << k;
        }
        sPw[(SB - 1) * PS] = hw; sP[(3 * SB - 1) * PS + lane] = hv; sP[(4 * SB - 1) * PS + lane] = hu;
        DEV_TRACE_MARK(2);   // phase A
        if (live != 0) {     // uniform
        wave_lds_sync();          // panel rows visible
        // ---------------- phase B: panel x Mom on the matrix pipe ----------------
        // D layout: lane l, register r -> row 4 (l >> 4) + r, column l & 15
        // (lane-derived addresses are re-derived here every block: hoisted out of the loop they would hold ~20 VGPRs across phase A)
        int lB = lane;
        BWDP_OPAQUE(lB);
        const int colB = lB & 15, grpB = lB >> 4;
        const int cq = lB & 7, jq = lB >> 3;   // geometric epilogue: lane = (value j, candidate c)
        f32x4 accM = {0.f, 0.f, 0.f, 0.f};
        float4 Aq, Bq;
        float DBq;
        {   // rows (v | u) x Mom: lanes 0..31, columns 0..5 = the six pixel moments of v; lanes 32..63, column 0 = sum of u
            const float4* ap = reinterpret_cast<const float4*>(sP + (2 * SB + colB) * PS + 16 * grpB);
            const float4 a0 = ap[0], a1 = ap[1], a2 = ap[2], a3 = ap[3];
            const float av[16] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w,
                                  a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
            // The epilogue's constants leave the record buffer now: behind these reads nothing of this block is left in it, and
            // the copy of the next block's records runs under the MFMAs below
            Aq = sC[cq]; Bq = sC[SB + cq]; DBq = sC[3 * SB + cq].x;
            if (more) {
                __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): every read of the buffer has returned
                stage_records(c0 + SB);
            }
            float c0l = cx0;
            BWDP_OPAQUE(c0l);   // (opaque: the 16 operand values are not hoisted out of the block loop into 16 VGPRs)
            f32x4 accM2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 16; kk++) {
                const float mx = (float)(kk & 7) - 3.5f;
                f32x4& acc = (BWDP_MFMA_ACC == 2 && (kk & 1)) ? accM2 : accM;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], (c0l + mx * (cx1 + mx * cx2)) * momy[kk >> 3], acc, 0, 0, 0);
            }
            if (BWDP_MFMA_ACC == 2) accM += accM2;
        }
        if (grpB < 2) {
            if (colB < 6) {
#pragma unroll
                for (int rr = 0; rr < 4; rr++) sM[(4 * grpB + rr) * 8 + colB] = accM[rr];
            }
        } else if (colB == 0) {
#pragma unroll
            for (int rr = 0; rr < 4; rr++) sM[(4 * (grpB - 2) + rr) * 8 + 6] = accM[rr];
        }
        // vmcnt(0): the next block's records have landed in LDS (issued in front of the MFMAs), and no atomic younger than a whole
        // phase is outstanding.  In FRONT of this block's atomics: vmcnt counts them too, and they do not retire in order with loads
        __builtin_amdgcn_s_waitcnt(0x0f70);
        wave_lds_sync();
        DEV_TRACE_MARK(3);   // phase B (MFMA)
        // lane = (value j = lane >> 3, candidate c = lane & 7): the six geometric gradients from the moments
        {
            if (jq < 6 && ((live >> cq) & 1u)) {
                const float4 m03 = *reinterpret_cast<const float4*>(sM + cq * 8);
                const float4 m47 = *reinterpret_cast<const float4*>(sM + cq * 8 + 4);
                const float Xc = Aq.x - cxs, Yc = Aq.y - cys;       // mean relative to the sub-tile centre
                const float M0 = m03.x, M1 = m03.y, M2 = m03.z, M3 = m03.w, M4 = m47.x, M5 = m47.y, Q = m47.z;
                const float Sx = Xc * M0 - M1, Sy = Yc * M0 - M2;  // sum v dx, sum v dy
                const float hf = Bq.y * -0.5f;                      // dL_ddist = v * hf
                float ge;
                // (the fused forms of a b + c d written out, as in phase A)
                if (jq == 0) ge = __builtin_fmaf(Q, Bq.w, hf * 2.f * __builtin_fmaf(Aq.w, Sy, Aq.z * Sx) * ddelx_dx);
                else if (jq == 1) ge = __builtin_fmaf(Q, DBq, hf * 2.f * __builtin_fmaf(Aq.w, Sx, Bq.x * Sy) * ddely_dy);
                else if (jq == 2) ge = hf * (Xc * (Sx - M1) + M3);              // sum v dx^2
                else if (jq == 3) ge = hf * ((Xc * Sy - Yc * M1) + M4);          // sum v dx dy
                else if (jq == 4) ge = hf * (Yc * (Sy - M2) + M5);              // sum v dy^2
                else ge = M0;
                if (ge != 0.f) atomic_add_f32(a.grad_rows + (uint32_t)(sQ[c0 + cq].x * (uint32_t)RS + (uint32_t)(GEO + jq)), ge);
            }
        }
        wave_lds_sync();   // moments / panel consumed before they are overwritten
        } else if (more) {   // nothing blends in this block: phase B is skipped, the next phase A still needs its records
            __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
            stage_records(c0 + SB);
            __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
            wave_lds_sync();
        }
        live16 = par ? (live16 | (live << SB)) : live;
        if ((par || c0 + SB >= nent) && live16 != 0) {   // (uniform) the pair is complete, or the segment ends on its first block
            wave_lds_sync();          // weight rows visible
            // ---------------- rows (w_a | w_b) x G: the channel gradients of the pair's 16 candidates, row = 8 (block of the pair) + k ----------------
            int lP = lane;
            BWDP_OPAQUE(lP);
            const int colP = lP & 15, grpP = lP >> 4;
            f32x4 accP = {0.f, 0.f, 0.f, 0.f};
            {
                const float4* ap = reinterpret_cast<const float4*>(sP + colP * PS + 16 * grpP);
                const float4 a0 = ap[0], a1 = ap[1], a2 = ap[2], a3 = ap[3];
                const float av[16] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w,
                                      a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
                f32x4 accP2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 16; kk++) {
                    f32x4& acc = (BWDP_MFMA_ACC == 2 && (kk & 1)) ? accP2 : accP;
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], Bp[kk], acc, 0, 0, 0);
                }
                if (BWDP_MFMA_ACC == 2) accP += accP2;
            }
            const int cp0 = c0 - par * SB;   // first candidate of the pair
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int cB = 4 * grpP + rr;   // (rows of a block that did not run, or without a blending pixel, are masked: never read as results)
                const bool mine = ((live16 >> cB) & 1u) && colP < NC0 && accP[rr] != 0.f;
                if (mine) atomic_add_f32(a.grad_rows + (uint32_t)(sQ[cp0 + cB].x * (uint32_t)RS + (uint32_t)colP), accP[rr]);
            }
            wave_lds_sync();   // weight rows consumed before the next pair overwrites them
        }
        DEV_TRACE_MARK(1);   // geometric epilogue
    }
    }   // loop over live segments
    DEV_TRACE_END(1, dev_items, dev_cands, blockIdx.x);
}

template <int S, bool SVGSS>
void launch(const RenderBwdArgs& a, hipStream_t s) {
    using PG = PlainGeom<S>;
    // one wave per live segment up to a few waves per resident slot; waves beyond the (device-side) count exit at once
    const int grid = std::max(8, std::min(a.seg_cap, BWDP_GRID_MULT * 256 * 4 * BWDP_WPE) & ~7);   // a multiple of 8: work id & 7 = XCD in every round
    hipLaunchKernelGGL((render_bwd_plain_kernel<S, SVGSS>), dim3(grid), dim3(64), PG::lds_bytes, s, a);
}

}  // namespace

int launch_render_bwd_plain(const RenderBwdArgs& a, bool svgss, hipStream_t s) {
    if (a.VS != 0) return -1;
#define CASE(SV, SG) if (a.S == SV && svgss == SG) { launch<SV, SG>(a, s); return 0; }
    CASE(0, true) CASE(5, true) CASE(0, false) CASE(5, false) CASE(3, false) CASE(1, false)
#undef CASE
    return -1;
}

#if defined(SVGIR_DEV)
extern "C" int svgir_dev_trace_read_bwd_plain(unsigned long long* out, int cap_records) {
    unsigned int n[2];
    if (hipMemcpyFromSymbol(n, HIP_SYMBOL(svgir::g_dev_trace_n), sizeof(n)) != hipSuccess) return -1;
    int cnt = (int)std::min<unsigned>(n[1], (unsigned)std::min(cap_records, svgir::DEV_TRACE_CAP));
    if (cnt > 0 && hipMemcpyFromSymbol(out, HIP_SYMBOL(svgir::g_dev_trace), (size_t)cnt * svgir::DEV_TRACE_WORDS * 8,
                                       (size_t)svgir::DEV_TRACE_CAP * svgir::DEV_TRACE_WORDS * 8) != hipSuccess) return -1;
    n[1] = 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(svgir::g_dev_trace_n), n, sizeof(n));
    return cnt;
}
#endif

}  // namespace svgir
