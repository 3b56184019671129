// epi_lines.hip -- the line aggregation of the calc_cost_sgm path (calc_cost_sgm.cpp:33-66 sgm_step, :86-257 sgm): one launch for
// every path direction of every frame, per-path cost volumes L_r in HBM for the WTA kernels (epi_wta.hip).  Here: the classes with
// 16 costs a lane (D = 16 << k) with their hand-written steps, the generic kernel for any D, and launch_aggregate with the lookups
// of FSGM_LINE_CLASSES (epi_kernels.h).  The general body is in epi_lines.h, the classes D = 48 .. 224 in epi_lines_split.hip.
#include "epi_lines.h"
#include <type_traits>
#include "epi_step.h"

namespace fsgm {

// =============================================================================================
// Along-x lines, D = 32 / 64 / 128, no wrap: the chain that bounds a single call (W steps, 2 H lines a frame -- fewer waves than the
// chip has SIMDs, so a step costs what its instructions cost a lone wave: 7.5-10 cycles each, profiles/r02_ubench_pk_rates.txt).
// Two costs a lane (D = 128: one line a wave; 64: two; 32: four), and the step written out by hand, 18 vector instructions (17 / 21
// at D = 32 / 64) where the general body above takes 55:
//  * the minimum over d comes out of the reduction as a replicated 2 x u16 in a scalar register (v_pk_min with op_sel folds
//    the halves, four row DPP stages, row_bcast:15/31, v_readlane): no broadcast, no select, usable as an operand directly;
//  * the neighbours L[d-1] + P1, L[d+1] + P1 come from whole-wave shifts into two registers whose lane 0 / lane 63 hold the
//    "no such neighbour" value for the whole line (a shift never writes them), and min(L[d], L[d-1] + P1, L[d+1] + P1) is one
//    v_pk_minimum3_f16 whose op_sel picks the halves (exact on these denormal patterns: self-tested at plan creation);
//  * the half of the next step that does not need the minimum fills the wait states between the reduction's DPP stages;
//  * addresses are immediate offsets from one register per 32 steps (32 x 128 bytes = the 4 KB immediate range).
// (D = 64: the minimum of a line's two rows through v_permlane16_swap into a vector register, the cross-line lanes of the shifts
// masked; D = 32: row shifts and the four row stages only.)  Same results as agg_packed_body<D, 4, false, 0>.
// =============================================================================================
#ifndef FSGM_AGG_XLEAN
#define FSGM_AGG_XLEAN 1
#endif

template <int D, bool MIRROR>
__device__ __forceinline__ void agg_x_lean_body(const AggArgs& a, const int slot) {
    constexpr int LPP = D / 2, PXW = 64 / LPP, PF = 32;        // two costs a lane; lines per wave
    static_assert(D == 32 || D == 64 || D == 128, "hand-written along-x step: 16, 32 or 64 lanes a line");
    constexpr int STEP = MIRROR ? -D : D;
    constexpr uint32_t SENT = 0x03FF03FFu;                     // "no neighbour": above every L + P1 (<= 510), below the fp16 normals
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPP, j = lane % LPP;
    const int W = a.W, H = a.H;
    const int lg = ((int)blockIdx.x - a.blk_begin[slot]) * 4 + wave;
    if (lg * PXW >= H) return;                                 // wave-uniform
    const int line = min(lg * PXW + g, H - 1);                 // lanes past the last line redo it (same loads, same stores)
    // pass 0 walks row `line` left to right; the mirrored pass walks pixel NP-1-pix: row H-1-line right to left
    const size_t first = MIRROR ? (size_t)W * H - 1 - (size_t)line * W : (size_t)line * W;
    const uint8_t* __restrict__ cp = a.C + (size_t)blockIdx.y * a.c_frame_stride + first * D + 2 * j;
    uint8_t* __restrict__ lp = a.L + (size_t)blockIdx.y * a.l_frame_stride + (size_t)slot * a.l_dir_stride + first * D + 2 * j;

    const uint32_t P1pk = (uint32_t)a.P1 * 0x10001u, P2pk = (uint32_t)a.P2 * 0x10001u;
    const uint32_t selc = 0x0C010C00u;     // u16 {c0, c1} -> 2 x u16
    const uint32_t selo = 0x0C0C0200u;     // 2 x u16 -> u16 of two bytes
    const uint32_t mL = j == 0 ? SENT : 0u, mR = j == LPP - 1 ? SENT : 0u;    // (32 lanes a line: the whole-wave shifts cross into the other line)
    uint32_t T = 0, CE, PR = SENT, NR = SENT, sm = 0, M = 0;

    // step t: phase B (needs the previous minimum) + reduction, with phase A of step t+1 in the reduction's wait states.
    // T: min(L[d], L[d-1] + P1, L[d+1] + P1) of the previous pixel; CE: this pixel's costs; cn: the next pixel's, raw.
    // The previous minimum, replicated in both halves: a scalar register with 64 lanes a line (M unused), the vector register M below.
#define FSGM_XLEAN_HEAD(MIN) \
            "v_pk_sub_u16 %[T], %[T], " MIN "\n\t" \
            "v_pk_min_u16 %[T], %[T], %[P2]\n\t" \
            "v_pk_add_u16 %[CUR], %[T], %[CE]\n\t" \
            "v_pk_min_u16 %[X], %[CUR], %[CUR] op_sel:[0,1] op_sel_hi:[1,0]\n\t" \
            "v_pk_add_u16 %[CP], %[CUR], %[P1]\n\t" \
            "v_perm_b32 %[O], %[CUR], %[CUR], %[SELO]\n\t" \
            "v_min_u32_dpp %[X], %[X], %[X] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" \
            "v_perm_b32 %[CE], %[CN], %[CN], %[SELC]\n\t"
    auto block = [&](const uint32_t cn, const uint32_t p2) -> uint32_t {
        uint32_t CUR, X, O, CP, NB;
        if constexpr (LPP == 64) {
            asm volatile(
                FSGM_XLEAN_HEAD("%[SM]")
                "v_mov_b32_dpp %[PR], %[CP] wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                "v_min_u32_dpp %[X], %[X], %[X] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                "v_mov_b32_dpp %[NR], %[CP] wave_shl:1 row_mask:0xf bank_mask:0xf\n\t"
                "s_nop 0\n\t"
                "v_min_u32_dpp %[X], %[X], %[X] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
                "v_alignbit_b32 %[NB], %[NR], %[PR], 16\n\t"
                "s_nop 0\n\t"
                "v_min_u32_dpp %[X], %[X], %[X] row_mirror row_mask:0xf bank_mask:0xf\n\t"
                "v_pk_minimum3_f16 %[T], %[CUR], %[CP], %[NB] op_sel:[0,1,0] op_sel_hi:[1,0,1]\n\t"
                "s_nop 0\n\t"
                "v_min_u32_dpp %[X], %[X], %[X] row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                "s_nop 1\n\t"
                "v_min_u32_dpp %[X], %[X], %[X] row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                "s_nop 1\n\t"
                "v_readlane_b32 %[SM], %[X], 63\n\t"
                "s_nop 1"
                : [T] "+v"(T), [CE] "+v"(CE), [PR] "+v"(PR), [NR] "+v"(NR), [SM] "+s"(sm),
                  [CUR] "=&v"(CUR), [X] "=&v"(X), [O] "=&v"(O), [CP] "=&v"(CP), [NB] "=&v"(NB)
                : [CN] "v"(cn), [P2] "s"(p2), [P1] "s"(P1pk), [SELO] "s"(selo), [SELC] "s"(selc));
        } else if constexpr (LPP == 32) {
            // two lines a wave: the shifted-in neighbours of a line's first / last lane are masked to "none", the minimum of a
            // line's two rows meets through a row swap and stays in a vector register
            uint32_t Y;
            asm volatile(
                FSGM_XLEAN_HEAD("%[M]")
                "v_mov_b32_dpp %[PR], %[CP] wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                "v_min_u32_dpp %[X], %[X], %[X] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                "v_mov_b32_dpp %[NR], %[CP] wave_shl:1 row_mask:0xf bank_mask:0xf\n\t"
                "v_or_b32 %[PR], %[PR], %[ML]\n\t"
                "v_min_u32_dpp %[X], %[X], %[X] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
                "v_or_b32 %[NR], %[NR], %[MR]\n\t"
                "v_alignbit_b32 %[NB], %[NR], %[PR], 16\n\t"
                "v_min_u32_dpp %[X], %[X], %[X] row_mirror row_mask:0xf bank_mask:0xf\n\t"
                "v_pk_minimum3_f16 %[T], %[CUR], %[CP], %[NB] op_sel:[0,1,0] op_sel_hi:[1,0,1]\n\t"
                "s_nop 0\n\t"
                "v_mov_b32 %[Y], %[X]\n\t"
                "s_nop 1\n\t"
                "v_permlane16_swap_b32 %[X], %[Y]\n\t"
                "s_nop 0\n\t"
                "v_min_u32 %[M], %[X], %[Y]"
                : [T] "+v"(T), [CE] "+v"(CE), [PR] "+v"(PR), [NR] "+v"(NR), [M] "+v"(M),
                  [CUR] "=&v"(CUR), [X] "=&v"(X), [Y] "=&v"(Y), [O] "=&v"(O), [CP] "=&v"(CP), [NB] "=&v"(NB)
                : [CN] "v"(cn), [P2] "s"(p2), [P1] "s"(P1pk), [SELO] "s"(selo), [SELC] "s"(selc), [ML] "v"(mL), [MR] "v"(mR));
        } else {
            // four lines a wave, a row each: row shifts never write a row's first / last lane, the row stages are the whole reduction
            asm volatile(
                FSGM_XLEAN_HEAD("%[M]")
                "v_mov_b32_dpp %[PR], %[CP] row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                "v_min_u32_dpp %[X], %[X], %[X] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                "v_mov_b32_dpp %[NR], %[CP] row_shl:1 row_mask:0xf bank_mask:0xf\n\t"
                "s_nop 0\n\t"
                "v_min_u32_dpp %[X], %[X], %[X] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
                "v_alignbit_b32 %[NB], %[NR], %[PR], 16\n\t"
                "s_nop 0\n\t"
                "v_min_u32_dpp %[M], %[X], %[X] row_mirror row_mask:0xf bank_mask:0xf\n\t"
                "v_pk_minimum3_f16 %[T], %[CUR], %[CP], %[NB] op_sel:[0,1,0] op_sel_hi:[1,0,1]"
                : [T] "+v"(T), [CE] "+v"(CE), [PR] "+v"(PR), [NR] "+v"(NR), [M] "+v"(M),
                  [CUR] "=&v"(CUR), [X] "=&v"(X), [O] "=&v"(O), [CP] "=&v"(CP), [NB] "=&v"(NB)
                : [CN] "v"(cn), [P2] "s"(p2), [P1] "s"(P1pk), [SELO] "s"(selo), [SELC] "s"(selc));
        }
        return O;
    };
#undef FSGM_XLEAN_HEAD
    auto ld = [&](const int t) -> uint32_t { return *(const uint16_t*)(cp + (ptrdiff_t)t * STEP); };
    auto st = [&](const int t, const uint32_t o) {
        if (FSGM_LINE_NT) __builtin_nontemporal_store((uint16_t)o, (uint16_t*)(lp + (ptrdiff_t)t * STEP));
        else *(uint16_t*)(lp + (ptrdiff_t)t * STEP) = (uint16_t)o;
    };

    // path start (calc_cost_sgm.cpp:154,164): L = C, stored minimum 0
    CE = __builtin_amdgcn_perm(0u, ld(0), selc);
    uint32_t ring[PF];                                         // ring[i]: the costs of step u0 + i + 2 (u = t - 1)
#pragma unroll
    for (int i = 0; i < PF; i++) ring[i] = ld(min(i + 2, W - 1));
    st(0, block(ld(min(1, W - 1)), 0u));
    sm = 0; M = 0;

    const int n = W - 1;                                       // steps u = 0..n-1 are pixels t = u + 1
    int u0 = 0;
    for (; u0 + 2 * PF + 2 <= W; u0 += PF) {                   // every load of the chunk inside the line; at most 2 PF steps are left after it
        const uint8_t* cq = cp + (ptrdiff_t)(u0 + 2 + PF) * STEP;
        uint8_t* lq = lp + (ptrdiff_t)(u0 + 1) * STEP;
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const uint32_t o = block(ring[i], P2pk);
            ring[i] = *(const uint16_t*)(cq + i * STEP);
            if (FSGM_LINE_NT) __builtin_nontemporal_store((uint16_t)o, (uint16_t*)(lq + i * STEP));
            else *(uint16_t*)(lq + i * STEP) = (uint16_t)o;
        }
    }
#pragma unroll
    for (int i = 0; i < PF; i++) {
        if (u0 + i < n) {
            const uint32_t cn = ring[i];
            if (u0 + i + 2 + PF < W) ring[i] = ld(u0 + i + 2 + PF);
            st(u0 + i + 1, block(cn, P2pk));
        }
    }
    u0 += PF;
#pragma unroll
    for (int i = 0; i < PF; i++)
        if (u0 + i < n) st(u0 + i + 1, block(ring[i], P2pk));
}

// =============================================================================================
// The other three directions (along y and the two diagonals), no wrap, 16 costs a lane: the general body with what a
// step does not need taken out -- these lines are most of a single call's instructions (6 of 8 slots), and with a few
// waves a SIMD an instruction costs 5-8 cycles whatever it does:
//  * min(L[d], L[d-1] + P1, L[d+1] + P1) as one v_pk_minimum3_f16 a register (exact on these denormal patterns: self-tested
//    at plan creation) on L + P1 aligned once, instead of align / min / add / min;
//  * the minimum over d leaves the reduction replicated in both halves (v_pk_min with op_sel folds them): no extract, no
//    re-broadcast;
//  * byte offsets advance by a constant (along y) or by one of two constants chosen by a down-counter (diagonals), the loads
//    stop at the line's end instead of being clamped, and a path start is the wrap of the previous advance.
// Same results as agg_packed_body<D, 16, false, BASE> (tests/test_gpu_epi.py runs both).
// =============================================================================================
#ifndef FSGM_AGG_LEAN
#define FSGM_AGG_LEAN 1
#endif
__device__ __forceinline__ uint32_t pk_min_fold(uint32_t x) {       // min(x.lo, x.hi) in both halves
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0]" : "=v"(r) : "v"(x));
    return r;
}
template <int D, int BASE>
__device__ __forceinline__ void agg_lean_body(const AggArgs& a, const int slot, const bool mirror) {
    constexpr int LPP = D / 16, PXW = 64 / LPP, PF = 4;
    constexpr uint32_t SENT = 0x03FF03FFu, MASK = 0x00FF00FFu;   // "no neighbour": above every L + P1, a denormal pattern
    static_assert(BASE >= 1 && BASE <= 3 && LPP >= 2 && LPP <= 16, "lean body: along y / diagonals, D = 32..256");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPP, j = lane % LPP;
    const int W = a.W, H = a.H, NP = W * H, len = H;
    const int lg = ((int)blockIdx.x - a.blk_begin[slot]) * 4 + wave;
    if (lg * PXW >= W) return;                               // wave-uniform
    const int l = min(lg * PXW + g, W - 1);                  // lanes past the last line redo it (same loads, same stores)

    const uint8_t* __restrict__ Cf = a.C + (size_t)blockIdx.y * a.c_frame_stride;
    uint8_t* __restrict__ Lf = a.L + (size_t)blockIdx.y * a.l_frame_stride + (size_t)slot * a.l_dir_stride;
    // byte offset of this lane's 16 costs at the pass-0 pixel `pix`; the mirrored pass addresses NP-1-pix
    const int sgn = mirror ? -1 : 1;
    const uint32_t dN = (uint32_t)(sgn * (W + (BASE == 2 ? 1 : BASE == 3 ? -1 : 0)) * D);    // a step inside the frame
    const uint32_t dW = (uint32_t)(sgn * (BASE == 2 ? 1 : 2 * W - 1) * D);                   // the step that wraps in x
    uint32_t oc = (uint32_t)(mirror ? NP - 1 - l : l) * D + (uint32_t)j * 16, ol = oc;        // compute / load cursors
    int cc = BASE == 2 ? W - l : l + 1, cl = cc;                                             // advances until the wrap
    // advance a cursor; true where it wrapped (the pixel reached starts a new path, calc_cost_sgm.cpp:154-177)
    auto adv = [&](uint32_t& o, int& c) -> bool {
        if (BASE == 1) { o += dN; return false; }
        c -= 1;
        const bool wr = c == 0;
        c = wr ? W : c;
        o += wr ? dW : dN;
        return wr;
    };
    auto load_c = [&](uint32_t o) -> uint4 { return *(const uint4*)(Cf + o); };
    auto store_l = [&](uint32_t o, const uint4& v) {
        if (FSGM_LINE_NT) store_nt(Lf + o, v); else *(uint4*)(Lf + o) = v;
    };

    const uint32_t P1pk = (uint32_t)a.P1 * 0x10001u, P2pk = (uint32_t)a.P2 * 0x10001u;
    const uint32_t mL = j == 0 ? SENT : 0u, mR = j == LPP - 1 ? SENT : 0u;
    uint32_t LE[4], LO[4], m = 0, pr = SENT, nr = SENT;
#pragma unroll
    for (int k = 0; k < 4; k++) LE[k] = LO[k] = 0;

    // one step; FIRST: the line's first pixel (every lane starts a path); start: lanes whose previous advance wrapped
    auto step = [&](const uint4 raw, auto first, const bool start) -> uint4 {
        constexpr bool FIRST = decltype(first)::value;
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
        uint32_t CE[4], CO[4], NE[4], NO[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { CE[k] = w[k] & MASK; CO[k] = __builtin_amdgcn_perm(0u, w[k], 0x0C030C01u); }
        if (FIRST) {
#pragma unroll
            for (int k = 0; k < 4; k++) { NE[k] = CE[k]; NO[k] = CO[k]; }
            m = 0;
        } else {
            uint32_t EP[4], OP[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { EP[k] = pk_add(LE[k], P1pk); OP[k] = pk_add(LO[k], P1pk); }
            // the neighbouring lanes' d-1 / d+1 (the first lane of a row of 16 keeps SENT: a row shift never writes it)
            asm("s_nop 1\n\tv_mov_b32_dpp %0, %1 row_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(pr) : "v"(OP[3]));
            asm("s_nop 1\n\tv_mov_b32_dpp %0, %1 row_shl:1 row_mask:0xf bank_mask:0xf" : "+v"(nr) : "v"(EP[0]));
            const uint32_t prevOP = LPP == 16 ? pr : (pr | mL), nextEP = LPP == 16 ? nr : (nr | mR);
            const uint32_t p2lane = (BASE != 1 && start) ? 0u : P2pk;       // min(., 0) = 0: L = C at a path start
            uint32_t mk[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t tE = pk_min3(LE[k], align16(OP[k], k ? OP[k - 1] : prevOP), OP[k]);
                const uint32_t tO = pk_min3(LO[k], EP[k], align16(k < 3 ? EP[k + 1] : nextEP, EP[k]));
                NE[k] = pk_add(CE[k], pk_min(pk_sub(tE, m), p2lane));      // C + min(t - m, P2): t >= m without wrap
                NO[k] = pk_add(CO[k], pk_min(pk_sub(tO, m), p2lane));
                mk[k] = pk_min(NE[k], NO[k]);
            }
            const uint32_t mx = group_min_u32<LPP>(pk_min_fold(pk_min(pk_min(mk[0], mk[1]), pk_min(mk[2], mk[3]))));
            m = (BASE != 1 && start) ? 0u : mx;                            // stored minimum 0 at a path start
        }
        uint4 o;
        uint32_t ow[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            LE[k] = NE[k]; LO[k] = NO[k];
            ow[k] = __builtin_amdgcn_perm(NO[k], NE[k], 0x06020400u);       // bytes E.lo, O.lo, E.hi, O.hi
        }
        o.x = ow[0]; o.y = ow[1]; o.z = ow[2]; o.w = ow[3];
        return o;
    };

    // first pixel, then steps u = t - 1 = 0..n-1 with the ring PF steps ahead
    store_l(oc, step(load_c(ol), std::true_type{}, true));
    bool wrapped = adv(oc, cc);
    adv(ol, cl);
    const int n = len - 1;
    uint4 ring[PF];
#pragma unroll
    for (int i = 0; i < PF; i++) {
        if (i < n) { ring[i] = load_c(ol); adv(ol, cl); } else ring[i] = make_uint4(0, 0, 0, 0);
    }
    int u0 = 0;
    for (; u0 + 2 * PF <= n; u0 += PF) {
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const uint4 cw = ring[i];
            ring[i] = load_c(ol);
            adv(ol, cl);
            store_l(oc, step(cw, std::false_type{}, wrapped));
            wrapped = adv(oc, cc);
        }
    }
#pragma unroll
    for (int i = 0; i < PF; i++) {
        if (u0 + i < n) {
            const uint4 cw = ring[i];
            if (u0 + i + PF < n) { ring[i] = load_c(ol); adv(ol, cl); }
            store_l(oc, step(cw, std::false_type{}, wrapped));
            wrapped = adv(oc, cc);
        }
    }
    u0 += PF;
#pragma unroll
    for (int i = 0; i < PF; i++) {
        if (u0 + i < n) {
            store_l(oc, step(ring[i], std::false_type{}, wrapped));
            wrapped = adv(oc, cc);
        }
    }
}

// The along-x lines are the long serial chains (W steps against H for every other direction) and there are
// few of them (2 H lines a frame): split finer over the lanes, 4 costs a lane (8 at D = 256), they take a
// third of the instructions per step; every other direction keeps 16 costs a lane.
#ifndef FSGM_AGG_DX
#define FSGM_AGG_DX 4
#endif
#ifndef FSGM_AGG_DO
#define FSGM_AGG_DO 16
#endif
template <int D> struct AggSplit {
    static constexpr int along_x = D >= 256 && FSGM_AGG_DX < 8 ? 8 : FSGM_AGG_DX;
    static constexpr int other = D >= 256 && FSGM_AGG_DO < 8 ? 8 : FSGM_AGG_DO;
};

// ADAPT: every direction on the general body (the hand-written bodies have no per-step P2), the along-x lines split finely
// EXACT: the same (the hand-written bodies' sentinels and fp16 minima are sized for the no-wrap budget, and they store L)
template <int D, bool WRAP, bool FINE, bool ADAPT, bool EXACT = false>
__device__ __forceinline__ void agg_packed_dispatch(const AggArgs& a) {
    // which direction slot does this block belong to (block-uniform)
    int slot = 0;
#pragma unroll
    for (int i = 1; i < 8; i++)
        if (i < a.ndirs && (int)blockIdx.x >= a.blk_begin[i]) slot = i;
    const int code = a.dir_code[slot];
    const bool mirror = (code & 4) != 0;
    constexpr int DO = AggSplit<D>::other, DX = FINE ? AggSplit<D>::along_x : DO;
    switch (code & 3) {                 // 0: along x, 1: along y, 2: x+1,y+1, 3: x-1,y+1
        case 0:
            if constexpr ((D == 32 || D == 64 || D == 128) && !WRAP && FINE && FSGM_AGG_XLEAN && !ADAPT && !EXACT) {
                if (mirror) agg_x_lean_body<D, true>(a, slot); else agg_x_lean_body<D, false>(a, slot);
            } else agg_packed_body<D, DX, WRAP, 0, ADAPT, EXACT>(a, slot, mirror);
            break;
#define FSGM_AGG_OTHER(BASE) \
            if constexpr (!WRAP && DO == 16 && D >= 32 && D <= 256 && FSGM_AGG_LEAN && !ADAPT && !EXACT) agg_lean_body<D, BASE>(a, slot, mirror); \
            else agg_packed_body<D, DO, WRAP, BASE, ADAPT, EXACT>(a, slot, mirror);
        case 1: FSGM_AGG_OTHER(1) break;
        case 2: FSGM_AGG_OTHER(2) break;
        default: FSGM_AGG_OTHER(3) break;
#undef FSGM_AGG_OTHER
    }
}

template <int D, bool WRAP, bool FINE>
__global__ __launch_bounds__(256) void agg_packed_kernel(AggArgs a) { agg_packed_dispatch<D, WRAP, FINE, false>(a); }

template <int D, bool WRAP>
__global__ __launch_bounds__(256) void agg_packed_adaptive_kernel(AggArgs a) { agg_packed_dispatch<D, WRAP, true, true>(a); }

// exact path arithmetic (epi_lines.h, EXACT), with or without adaptive P2: kernels of their own, the ones above stay what they were
template <int D, bool ADAPT>
__global__ __launch_bounds__(256) void agg_packed_exact_kernel(AggArgs a) { agg_packed_dispatch<D, false, true, ADAPT, true>(a); }

// =============================================================================================
// Path aggregation, generic kernel: any D (<= FSGM_GENERIC_MAX_D), exact u8 semantics.
// One wave per line, Lpre/Lcur in LDS, lanes stride over d.  Correctness path for disparity
// ranges the packed kernel does not cover; not tuned.
// =============================================================================================
template <bool ADAPT>
__global__ __launch_bounds__(256) void agg_generic_kernel(AggArgs a) {
    __shared__ uint8_t sL[4][2][FSGM_GENERIC_MAX_D + 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int slot = 0;
#pragma unroll
    for (int i = 1; i < 8; i++)
        if (i < a.ndirs && (int)blockIdx.x >= a.blk_begin[i]) slot = i;
    const int code = a.dir_code[slot];
    const int base = code & 3;
    const bool mirror = (code & 4) != 0;
    const int W = a.W, H = a.H, D = a.D;
    const int NP = W * H;
    const int nlines = base == 0 ? H : W;
    const int len = base == 0 ? W : H;
    const int line = ((int)blockIdx.x - a.blk_begin[slot]) * 4 + wave;
    if (line >= nlines) return;                              // wave-uniform
    const uint8_t* __restrict__ Cf = a.C + (size_t)blockIdx.y * a.c_frame_stride;
    uint8_t* __restrict__ Lf = a.L + (size_t)blockIdx.y * a.l_frame_stride + (size_t)slot * a.l_dir_stride;
    int x = base >= 2 ? line : 0, pix = base == 0 ? line * W : line;
    const int dpix = base == 0 ? 1 : (base == 1 ? W : (base == 2 ? W + 1 : W - 1));
    uint8_t* pre = sL[wave][0];
    uint8_t* cur = sL[wave][1];
    uint32_t m = 0;
    const uint8_t* __restrict__ If = ADAPT ? a.I1 + (size_t)blockIdx.y * a.i_frame_stride : nullptr;
    int ipre = 0;                                            // ADAPT: the previous pixel of the path (unused at a path start)
    for (int t = 0; t < len; t++) {
        const bool start = (t == 0) || (base == 2 && x == 0) || (base == 3 && x == W - 1);
        const size_t off = (size_t)(mirror ? NP - 1 - pix : pix) * D;
        uint32_t lo = 255;
        bool edge = false;
        if constexpr (ADAPT) {                               // calc_cost_sgm.cpp:68-72
            const int icur = If[mirror ? NP - 1 - pix : pix];
            const int diff = icur - ipre;
            edge = (diff < 0 ? -diff : diff) > 25;
            ipre = icur;
        }
        const uint32_t jump = (m + (uint32_t)(edge ? a.P2 / 8 : a.P2)) & 0xFF;
        for (int d = lane; d < D; d += 64) {
            const uint32_t c = Cf[off + d];
            uint32_t v;
            if (start) {
                v = c;
            } else {
                uint32_t best = min(jump, (uint32_t)pre[d]);
                if (d > 0) best = min(best, ((uint32_t)pre[d - 1] + (uint32_t)a.P1) & 0xFF);
                if (d < D - 1) best = min(best, ((uint32_t)pre[d + 1] + (uint32_t)a.P1) & 0xFF);
                v = (c + best - m) & 0xFF;
            }
            cur[d] = (uint8_t)v;
            Lf[off + d] = (uint8_t)v;
            lo = min(lo, v);
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) lo = min(lo, (uint32_t)__shfl_xor((int)lo, s));
        m = start ? 0u : lo;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);                  // lgkmcnt(0): LDS writes visible to the wave
        uint8_t* tmp = pre; pre = cur; cur = tmp;
        pix += dpix;
        if (base == 2) { x++; if (x == W) { x = 0; pix -= W; } }
        else if (base == 3) { x--; if (x < 0) { x = W - 1; pix += W; } }
    }
}

// The generic kernel with exact path arithmetic (include/fsgm.h, "exact"): path costs as u16 in LDS, no narrowing anywhere, the
// true minimum over d; the path volume takes y = L - C (one byte, [0, P2]).  0 <= P1, P2 <= 255: L <= 510, every sum below 2^16.
template <bool ADAPT>
__global__ __launch_bounds__(256) void agg_generic_exact_kernel(AggArgs a) {
    __shared__ uint16_t sL[4][2][FSGM_GENERIC_MAX_D + 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int slot = 0;
#pragma unroll
    for (int i = 1; i < 8; i++)
        if (i < a.ndirs && (int)blockIdx.x >= a.blk_begin[i]) slot = i;
    const int code = a.dir_code[slot];
    const int base = code & 3;
    const bool mirror = (code & 4) != 0;
    const int W = a.W, H = a.H, D = a.D;
    const int NP = W * H;
    const int nlines = base == 0 ? H : W;
    const int len = base == 0 ? W : H;
    const int line = ((int)blockIdx.x - a.blk_begin[slot]) * 4 + wave;
    if (line >= nlines) return;                              // wave-uniform
    const uint8_t* __restrict__ Cf = a.C + (size_t)blockIdx.y * a.c_frame_stride;
    uint8_t* __restrict__ Lf = a.L + (size_t)blockIdx.y * a.l_frame_stride + (size_t)slot * a.l_dir_stride;
    int x = base >= 2 ? line : 0, pix = base == 0 ? line * W : line;
    const int dpix = base == 0 ? 1 : (base == 1 ? W : (base == 2 ? W + 1 : W - 1));
    uint16_t* pre = sL[wave][0];
    uint16_t* cur = sL[wave][1];
    uint32_t m = 0;
    const uint8_t* __restrict__ If = ADAPT ? a.I1 + (size_t)blockIdx.y * a.i_frame_stride : nullptr;
    int ipre = 0;                                            // ADAPT: the previous pixel of the path (unused at a path start)
    for (int t = 0; t < len; t++) {
        const bool start = (t == 0) || (base == 2 && x == 0) || (base == 3 && x == W - 1);
        const size_t off = (size_t)(mirror ? NP - 1 - pix : pix) * D;
        uint32_t lo = 0xFFFFFFFFu;
        bool edge = false;
        if constexpr (ADAPT) {                               // calc_cost_sgm.cpp:68-72
            const int icur = If[mirror ? NP - 1 - pix : pix];
            const int diff = icur - ipre;
            edge = (diff < 0 ? -diff : diff) > 25;
            ipre = icur;
        }
        const uint32_t p2 = (uint32_t)(edge ? a.P2 / 8 : a.P2);
        for (int d = lane; d < D; d += 64) {
            const uint32_t c = Cf[off + d];
            uint32_t y = 0;                                  // a path start: L = C
            if (!start) {
                uint32_t best = pre[d];
                if (d > 0) best = min(best, (uint32_t)pre[d - 1] + (uint32_t)a.P1);
                if (d < D - 1) best = min(best, (uint32_t)pre[d + 1] + (uint32_t)a.P1);
                y = min(best - m, p2);                       // best >= m: every candidate is a cost of the previous pixel or above one
            }
            cur[d] = (uint16_t)(c + y);
            Lf[off + d] = (uint8_t)y;
            lo = min(lo, c + y);
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) lo = min(lo, (uint32_t)__shfl_xor((int)lo, s));
        m = start ? 0u : lo;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);                  // lgkmcnt(0): LDS writes visible to the wave
        uint16_t* tmp = pre; pre = cur; cur = tmp;
        pix += dpix;
        if (base == 2) { x++; if (x == W) { x = 0; pix -= W; } }
        else if (base == 3) { x--; if (x < 0) { x = W - 1; pix += W; } }
    }
}

// =============================================================================================
// launchers and the lookups of FSGM_LINE_CLASSES
// =============================================================================================
// How the general line kernels and the packed WTA split D over the lanes of a pixel: the class's row, false for every other D
bool agg_line_split(int D, int* lpp, int* dpl) {
    int l = 0, c = 0;
    switch (D) {
#define FSGM_X(D, LPP, DPL) case D: l = LPP; c = DPL; break;
        FSGM_LINE_CLASSES(FSGM_X)
#undef FSGM_X
        default: return false;
    }
    if (lpp) *lpp = l;
    if (dpl) *dpl = c;
    return true;
}

int agg_packed_lpp(int D) {
    int l = 0, c = 0;
    return agg_line_split(D, &l, &c) && c == 16 ? l : 0;
}

// FSGM_AGG_FINE=0 keeps 16 costs a lane along x too (the round-1 split), for comparison
static bool agg_fine() {
    static const bool v = [] { const char* e = getenv("FSGM_AGG_FINE"); return !(e && e[0] == '0'); }();
    return v;
}

template <int D>
static void launch_packed(hipStream_t st, AggArgs& a, int paths, int frames, bool wrap) {
    constexpr int DO = AggSplit<D>::other, DX = AggSplit<D>::along_x;
    if (a.exact) {                                               // the general body for every direction, along x split finely
        plan_dirs(a, paths, 4 * (64 / (D / DX)), 4 * (64 / (D / DO)));
        dim3 grid(a.blk_begin[8], frames);
        if (a.adaptive) hipLaunchKernelGGL((agg_packed_exact_kernel<D, true>), grid, dim3(256), 0, st, a);
        else            hipLaunchKernelGGL((agg_packed_exact_kernel<D, false>), grid, dim3(256), 0, st, a);
        return;
    }
    if (a.adaptive) {                                            // the general body for every direction, along x split finely
        plan_dirs(a, paths, 4 * (64 / (D / DX)), 4 * (64 / (D / DO)));
        dim3 grid(a.blk_begin[8], frames);
        if (wrap) hipLaunchKernelGGL((agg_packed_adaptive_kernel<D, true>), grid, dim3(256), 0, st, a);
        else      hipLaunchKernelGGL((agg_packed_adaptive_kernel<D, false>), grid, dim3(256), 0, st, a);
        return;
    }
    const bool fine = agg_fine();
    const bool lean = (D == 32 || D == 64 || D == 128) && !wrap && fine && FSGM_AGG_XLEAN;      // agg_x_lean_body: two costs a lane
    plan_dirs(a, paths, lean ? 4 * (128 / D) : 4 * (64 / (D / (fine ? DX : DO))), 4 * (64 / (D / DO)));
    dim3 grid(a.blk_begin[8], frames);
    if (wrap) {
        if (fine) hipLaunchKernelGGL((agg_packed_kernel<D, true, true>), grid, dim3(256), 0, st, a);
        else      hipLaunchKernelGGL((agg_packed_kernel<D, true, false>), grid, dim3(256), 0, st, a);
    } else {
        if (fine) hipLaunchKernelGGL((agg_packed_kernel<D, false, true>), grid, dim3(256), 0, st, a);
        else      hipLaunchKernelGGL((agg_packed_kernel<D, false, false>), grid, dim3(256), 0, st, a);
    }
}

template <int D, int DPL>
static void launch_class(hipStream_t st, AggArgs& a, int paths, int frames, bool wrap) {
    if constexpr (DPL == 16) launch_packed<D>(st, a, paths, frames, wrap);
    else launch_split_lines(st, a, paths, frames, wrap);
}

void launch_aggregate(hipStream_t st, AggArgs a, int paths, int frames, int kernel_kind) {
    a.exact = kernel_kind == AGG_PACKED_EXACT || kernel_kind == AGG_GENERIC_EXACT;
    if (kernel_kind == AGG_GENERIC_EXACT) {
        plan_dirs(a, paths, 4, 4);
        dim3 grid(a.blk_begin[8], frames);
        if (a.adaptive) hipLaunchKernelGGL(agg_generic_exact_kernel<true>, grid, dim3(256), 0, st, a);
        else            hipLaunchKernelGGL(agg_generic_exact_kernel<false>, grid, dim3(256), 0, st, a);
        return;
    }
    if (kernel_kind == AGG_GENERIC) {
        plan_dirs(a, paths, 4, 4);
        dim3 grid(a.blk_begin[8], frames);
        if (a.adaptive) hipLaunchKernelGGL(agg_generic_kernel<true>, grid, dim3(256), 0, st, a);
        else            hipLaunchKernelGGL(agg_generic_kernel<false>, grid, dim3(256), 0, st, a);
        return;
    }
    const bool wrap = kernel_kind == AGG_PACKED_WRAP;
    switch (a.D) {
#define FSGM_X(D, LPP, DPL) case D: launch_class<D, DPL>(st, a, paths, frames, wrap); break;
        FSGM_LINE_CLASSES(FSGM_X)
#undef FSGM_X
        default: break;
    }
}

}  // namespace fsgm
