// epi_lines.h -- what the two units of the line aggregation share: the general body of a line and the plan of a launch's
// direction slots.  epi_lines.hip holds the classes with 16 costs a lane (and the generic kernel), epi_lines_split.hip the ones
// with 12, 20 or 28 (FSGM_LINE_CLASSES, epi_kernels.h); nothing else includes this.
#pragma once
#include "epi_kernels.h"
#include "fsgm_device.h"

namespace fsgm {

// =============================================================================================
// Path aggregation, packed kernel  (calc_cost_sgm.cpp:33-66 sgm_step, :86-257 sgm).
//
// One launch covers every path direction of every frame.  A path direction r has lines
// (rows for the horizontal paths, columns for the vertical ones, wrapped diagonals for the
// oblique ones); every line is an independent serial recurrence.  Lane layout inside a wave:
//   LPP = D/16 adjacent lanes own one pixel, 16 consecutive d each (one 16-byte load);
//   64/LPP adjacent lines advance in lockstep in one wave.
// The 16 costs of a lane live in 8 VGPRs as packed 2 x u16, split into even/odd bytes of each
// loaded dword:  E[k] = (d[4k], d[4k+2]),  O[k] = (d[4k+1], d[4k+3]).  With that split the
// d+1 neighbours of E[k] are O[k] itself and the d-1 neighbours of O[k] are E[k]; the other two
// neighbour vectors cost one v_alignbit each, and only the two lane-boundary elements need a DPP
// row shift.  The running minimum over d is a packed min tree + 3 DPP butterflies (LPP = 8).
//
// Path start (calc_cost_sgm.cpp:152-180): L = C and the stored minimum is 0 (not min C).
// A diagonal line that leaves the image re-enters at the opposite border as a new path, so all
// diagonal lines have H steps and a start wherever x hits the border.
//
// Pass 1 of the reference is the point mirror of pass 0 (:115-123), i.e. pixel index
// NP-1-idx; d is not mirrored.
//
// WRAP=false requires 0<=P1, 0<=P2, max(C)+P2+max(P1,P2) <= 255: then none of the reference's
// u8 narrowings changes a value and 16-bit lanes are exact.  WRAP=true reduces mod 256 at every
// point where the reference narrows to unsigned char.
//
// EXACT (with WRAP=false; include/fsgm.h, "exact"): the same 16-bit arithmetic with no budget -- 0 <= P1, P2 <= 255 and any
// costs.  Nothing narrows, so 0 <= L - C <= P2, L <= 255 + P2 <= 510, L + P1 <= 765 and t - m >= 0 (every candidate of t is a
// path cost of the previous pixel, at least its minimum m): no half of a register ever wraps.  The absent neighbours of d = 0
// and d = D-1 are 0xFFFF halves that meet a minimum with a real L BEFORE P1 is added, so they never turn into a small number.
// What goes to the path volume is y = L - C (one byte, [0, P2]) instead of L, which no longer fits one; the WTA adds C back.
// =============================================================================================
#ifndef FSGM_AGG_PFX
#define FSGM_AGG_PFX 16
#endif
#ifndef FSGM_AGG_PFO
#define FSGM_AGG_PFO 4
#endif

// ADAPT (adaptive P2, calc_cost_sgm.cpp:68-72 with adpativeP2 = true): a step uses P2 / 8 in place of P2 where the first image
// differs by more than 25 between the pixel and its predecessor on the path.  The pixel bytes ride with the cost words: one
// byte load a step into a ring of its own, PF steps ahead with the same clamped cursor (the LPP lanes of a pixel read the same
// byte: one request), the predecessor's byte carried in a register; the choice is a compare and a select, no branch.  A path
// start takes no step and reads no pair (:152-180), so what the carried byte holds there never matters.
template <int D, int DPL, bool WRAP, int BASE, bool ADAPT = false, bool EXACT = false>
__device__ __forceinline__ void agg_packed_body(const AggArgs& a, const int slot, const bool mirror) {
    constexpr int LPP = D / DPL;        // lanes per pixel
    constexpr int NK = DPL / 4;         // cost dwords per lane
    constexpr int PXW = 64 / LPP;       // lines per wave
    // prefetch depth (steps of C in flight per lane): the finely split along-x lines take a dword a step, and a step of theirs is
    // shorter than a quarter of the memory latency
    constexpr int PF = (BASE == 0 && NK == 1) ? FSGM_AGG_PFX : FSGM_AGG_PFO;
    constexpr uint32_t SENT = 0xFFFFFFFFu;
    constexpr uint32_t MASK = 0x00FF00FFu;
    static_assert(!(EXACT && WRAP), "exact arithmetic is the no-wrap form without its budget");
    static_assert(LPP >= 1 && LPP <= 32 && (LPP & (LPP - 1)) == 0 && DPL % 4 == 0 && NK >= 1 && NK <= 7 && (NK <= 2 || NK == 4 || LPP <= 16),
                  "lane split");
    // NK = 3, 5, 7 (D = 48 .. 224, agg_line_split): a lane's costs start at pix * D + j * DPL, a multiple of 4 only
    constexpr bool POW2 = (NK & (NK - 1)) == 0;
    struct __attribute__((aligned(POW2 ? NK * 4 : 4))) Words { uint32_t v[NK]; };

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPP, j = lane % LPP;

    const int W = a.W, H = a.H;
    const int NP = W * H;
    const int nlines = BASE == 0 ? H : W;
    const int len = BASE == 0 ? W : H;
    const int lg = ((int)blockIdx.x - a.blk_begin[slot]) * 4 + wave;
    if (lg * PXW >= nlines) return;                         // wave-uniform
    // Lanes past the last line redo the last line: they load the same bytes and store the same
    // bytes to the same addresses as its real lanes (which sit in this same wave), so the loop
    // needs no per-lane predicate.
    const int l = min(lg * PXW + g, nlines - 1);

    const uint8_t* __restrict__ Cf = a.C + (size_t)blockIdx.y * a.c_frame_stride;
    uint8_t* __restrict__ Lf = a.L + (size_t)blockIdx.y * a.l_frame_stride + (size_t)slot * a.l_dir_stride;

    // forward-frame cursors: (x, pix) for the compute side, (xl, pixl) PF steps ahead for loads.
    // pix is the pixel index in the pass-0 frame; pass 1 (mirror) addresses NP-1-pix.
    int x = BASE >= 2 ? l : 0, pix = BASE == 0 ? l * W : l;
    int xl = x, pixl = pix;

    auto advance = [&](int& cx, int& cpix) {               // branch-free
        if (BASE == 0) cpix += 1;
        if (BASE == 1) cpix += W;
        if (BASE == 2) { cx += 1; const bool wr = cx == W; cx = wr ? 0 : cx; cpix += wr ? 1 : W + 1; }
        if (BASE == 3) { cx -= 1; const bool wr = cx < 0; cx = wr ? W - 1 : cx; cpix += wr ? 2 * W - 1 : W - 1; }
    };
    auto byte_off = [&](int cpix) -> uint32_t {
        const int ap = mirror ? NP - 1 - cpix : cpix;
        return (uint32_t)ap * D + (uint32_t)j * DPL;
    };
    // the load cursor runs PF steps ahead of the line's end: keep its address inside the volume
    auto load_c = [&](int cpix) -> Words { return *(const Words*)(Cf + byte_off(min(cpix, NP - 1))); };
    const uint8_t* __restrict__ If = ADAPT ? a.I1 + (size_t)blockIdx.y * a.i_frame_stride : nullptr;
    auto load_i = [&](int cpix) -> uint32_t {              // the pixel of step cpix, clamped as load_c: index 0 .. NP-1
        const int q = min(cpix, NP - 1);
        return If[mirror ? NP - 1 - q : q];
    };
    // the path volumes are written once and read once by the WTA kernel: streamed past the caches (FSGM_LINE_NT)
    auto store_words = [&](uint8_t* p, const Words& w) {
        if constexpr (!POW2) {
            if (FSGM_LINE_NT) store_nt_words<NK>(p, w.v); else *(Words*)p = w;       // 4 + 2 + 1 dwords, each piece 4-byte aligned
        } else if (FSGM_LINE_NT) {
            typedef uint32_t wv __attribute__((ext_vector_type(NK)));
            wv t;
#pragma unroll
            for (int k = 0; k < NK; k++) t[k] = w.v[k];
            __builtin_nontemporal_store(t, (wv*)p);
        } else *(Words*)p = w;
    };

    const uint32_t P1pk = WRAP ? (uint32_t)(a.P1 & 0xFF) * 0x10001u : (uint32_t)a.P1 * 0x10001u;
    const uint32_t P2pk = (uint32_t)a.P2 * 0x10001u;        // NOWRAP only
    const uint32_t P2b = (uint32_t)(a.P2 & 0xFF);           // WRAP only
    const uint32_t P2apk = (uint32_t)(a.P2 / 8) * 0x10001u; // ADAPT: P2 / 8, C's truncating division (:71); NOWRAP (P2 >= 0)
    const uint32_t P2ab = (uint32_t)((a.P2 / 8) & 0xFF);    // ADAPT, WRAP
    uint32_t ipre = 0;                                       // ADAPT: the previous pixel of the path
    bool edge = false;                                       // ADAPT: the step being computed crosses an intensity edge and takes P2 / 8

    uint32_t LE[NK], LO[NK];                                 // previous pixel's path costs
#pragma unroll
    for (int k = 0; k < NK; k++) LE[k] = LO[k] = 0;
    uint32_t m = 0;                                          // previous pixel's stored minimum

    // one DP step on the DPL costs of this lane; returns the packed output dwords
    auto step = [&](const Words cw, const bool start) -> Words {
        uint32_t CE[NK], CO[NK];
#pragma unroll
        for (int k = 0; k < NK; k++) {
            CE[k] = __builtin_amdgcn_perm(0u, cw.v[k], 0x0C020C00u);   // bytes 0,2 -> 2 x u16
            CO[k] = __builtin_amdgcn_perm(0u, cw.v[k], 0x0C030C01u);   // bytes 1,3 -> 2 x u16
        }
        // lane-boundary neighbours (a pixel of 32 lanes spans two DPP rows: whole-wave shifts there)
        uint32_t prevO3 = LPP > 16 ? dpp_mov<DPP_WAVE_SHR1>(SENT, LO[NK - 1]) : dpp_mov<DPP_ROW_SHR1>(SENT, LO[NK - 1]);
        uint32_t nextE0 = LPP > 16 ? dpp_mov<DPP_WAVE_SHL1>(SENT, LE[0]) : dpp_mov<DPP_ROW_SHL1>(SENT, LE[0]);
        if (j == 0) prevO3 = SENT;                   // d = 0 has no d-1      (:47)
        if (j == LPP - 1) nextE0 = SENT;             // d = D-1 has no d+1    (:48)

        const uint32_t mpk = m | (m << 16);
        uint32_t NE[NK], NO[NK];
        uint32_t YE[EXACT ? NK : 1], YO[EXACT ? NK : 1];        // EXACT: y = L - C, what the path volume holds
        if (!WRAP) {
            const uint32_t p2lane = start ? 0u : (ADAPT && edge) ? P2apk : P2pk;   // min(.,0)=0 -> L = C at a path start
#pragma unroll
            for (int k = 0; k < NK; k++) {
                const uint32_t nbE = pk_min(align16(LO[k], k ? LO[k - 1] : prevO3), LO[k]);
                const uint32_t nbO = pk_min(LE[k], align16(k < NK - 1 ? LE[k + 1] : nextE0, LE[k]));
                const uint32_t tE = pk_min(LE[k], pk_add(nbE, P1pk));
                const uint32_t tO = pk_min(LO[k], pk_add(nbO, P1pk));
                // C + min(t, m+P2) - m  ==  C + min(t-m, P2)   (no wrap: t >= m)
                if constexpr (EXACT) {
                    YE[k] = pk_min(pk_sub(tE, mpk), p2lane);
                    YO[k] = pk_min(pk_sub(tO, mpk), p2lane);
                    NE[k] = pk_add(CE[k], YE[k]);
                    NO[k] = pk_add(CO[k], YO[k]);
                } else {
                    NE[k] = pk_add(CE[k], pk_min(pk_sub(tE, mpk), p2lane));
                    NO[k] = pk_add(CO[k], pk_min(pk_sub(tO, mpk), p2lane));
                }
            }
        } else {
            const uint32_t jump = (m + ((ADAPT && edge) ? P2ab : P2b)) & 0xFFu;   // :46 u8(LpreMin + P2)
            const uint32_t jpk = jump | (jump << 16);
            // mod-256 adds do not commute with min: narrow each neighbour + P1 first (:47-48),
            // and give the two non-existent neighbours the neutral candidate 255.
            const uint32_t noL = j == 0 ? 0x000000FFu : 0u;
            const uint32_t noR = j == LPP - 1 ? 0x00FF0000u : 0u;
#pragma unroll
            for (int k = 0; k < NK; k++) {
                const uint32_t lE = align16(LO[k], k ? LO[k - 1] : prevO3);            // d-1 of E[k]
                const uint32_t rO = align16(k < NK - 1 ? LE[k + 1] : nextE0, LE[k]);   // d+1 of O[k]
                uint32_t cEl = pk_add(lE, P1pk) & MASK;
                uint32_t cOr = pk_add(rO, P1pk) & MASK;
                if (k == 0) cEl |= noL;
                if (k == NK - 1) cOr |= noR;
                const uint32_t cEr = pk_add(LO[k], P1pk) & MASK;                     // d+1 of E[k] = O[k]
                const uint32_t cOl = pk_add(LE[k], P1pk) & MASK;                     // d-1 of O[k] = E[k]
                const uint32_t tE = pk_min(pk_min(LE[k], jpk), pk_min(cEl, cEr));
                const uint32_t tO = pk_min(pk_min(LO[k], jpk), pk_min(cOl, cOr));
                const uint32_t e = pk_sub(pk_add(CE[k], tE), mpk) & MASK;  // :60 mod 256
                const uint32_t o = pk_sub(pk_add(CO[k], tO), mpk) & MASK;
                NE[k] = start ? CE[k] : e;
                NO[k] = start ? CO[k] : o;
            }
        }
        // minimum over d of the new costs (:61,:65); 0 at a path start (:154,:164)
        uint32_t mk[NK];
#pragma unroll
        for (int k = 0; k < NK; k++) mk[k] = pk_min(NE[k], NO[k]);
#pragma unroll
        for (int w = 1; w < NK; w *= 2)
#pragma unroll
            for (int k = 0; k + w < NK; k += 2 * w) mk[k] = pk_min(mk[k], mk[k + w]);
        const uint32_t mm = mk[0];
        uint32_t mx = min(mm & 0xFFFFu, mm >> 16);
        mx = group_min_u32<LPP>(mx);
        m = start ? 0u : mx;
        Words o;
#pragma unroll
        for (int k = 0; k < NK; k++) {
            LE[k] = NE[k]; LO[k] = NO[k];
            if constexpr (EXACT) o.v[k] = __builtin_amdgcn_perm(YO[k], YE[k], 0x06020400u);
            else o.v[k] = __builtin_amdgcn_perm(NO[k], NE[k], 0x06020400u);  // bytes E.lo, O.lo, E.hi, O.hi
        }
        return o;
    };
    auto is_start = [&](int t) -> bool { return (t == 0) || (BASE == 2 && x == 0) || (BASE == 3 && x == W - 1); };

    // ADAPT: does the step onto pixel value icur cross an edge (:71); icur becomes the predecessor
    auto crosses = [&](const uint32_t icur) -> bool {
        const int diff = (int)icur - (int)ipre;
        ipre = icur;
        return (diff < 0 ? -diff : diff) > 25;
    };

    Words ring[PF];
    uint32_t iring[ADAPT ? PF : 1];                          // the pixels of the steps whose costs are in ring[]
#pragma unroll
    for (int i = 0; i < PF; i++) {
        ring[i] = load_c(pixl);
        if constexpr (ADAPT) iring[i] = load_i(pixl);
        advance(xl, pixl);
    }

    // steady state: no branches inside, so the PF loads stay in flight across iterations
    int t0 = 0;
    for (; t0 + PF <= len; t0 += PF) {
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const Words cw = ring[i];
            if constexpr (ADAPT) edge = crosses(iring[i]);
            ring[i] = load_c(pixl);
            if constexpr (ADAPT) iring[i] = load_i(pixl);
            advance(xl, pixl);
            const Words o = step(cw, is_start(t0 + i));
            store_words(Lf + byte_off(pix), o);
            advance(x, pix);
        }
    }
    // tail (len % PF steps): costs already in the ring
#pragma unroll
    for (int i = 0; i < PF - 1; i++) {
        if (t0 + i < len) {
            if constexpr (ADAPT) edge = crosses(iring[i]);
            const Words o = step(ring[i], is_start(t0 + i));
            store_words(Lf + byte_off(pix), o);
            advance(x, pix);
        }
    }
}

// Fill blk_begin / dir_code for `paths` directions.  Long (horizontal) lines first so that the
// W-step chains start before the H-step ones.
inline void plan_dirs(AggArgs& a, int paths, int lines_per_block_x, int lines_per_block) {
    static const int order8[8] = {0, 4, 1, 5, 2, 6, 3, 7};
    static const int order4[4] = {0, 4, 1, 5};      // also the 2-slot horizontal-only plan: {0, 4}
    a.ndirs = paths;
    int acc = 0;
    for (int i = 0; i < paths; i++) {
        const int code = paths == 8 ? order8[i] : order4[i];
        a.dir_code[i] = code;
        a.blk_begin[i] = acc;
        const int nlines = (code & 3) == 0 ? a.H : a.W;
        const int lpb = (code & 3) == 0 ? lines_per_block_x : lines_per_block;
        acc += (nlines + lpb - 1) / lpb;
    }
    for (int i = paths; i <= 8; i++) a.blk_begin[i] = acc;
    for (int i = paths; i < 8; i++) a.dir_code[i] = 0;
}

// the rows of FSGM_LINE_CLASSES with 12, 20 or 28 costs a lane (epi_lines_split.hip); launch_aggregate sends them there
// (a.exact: the exact kernels, wrap unused)
void launch_split_lines(hipStream_t st, AggArgs& a, int paths, int frames, bool wrap);

}  // namespace fsgm
