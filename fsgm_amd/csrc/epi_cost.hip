// epi_cost.hip -- the cost stage of calc_cost_sgm, every form of it and the selector between them (select_cost_kernels).
// First as ONE kernel: raw census cost along the epipolar line (calc_cost_sgm.cpp:343-381) and its 5x5 box mean with
// replicate border (:387-407) without the raw volume ever reaching HBM.  gfx950 only.  The two-kernel form -- a raw-cost
// kernel into a volume in HBM, then one of three box kernels -- follows it: every D the fused kernel does not take.
//
// Who does what.  A lane owns one pixel column x and 16 consecutive d; wave w of a workgroup owns d = 16 w .. 16 w + 15
// (D / 16 waves: 8 at D = 128), all waves the same 64 columns.  Neighbouring lanes are neighbouring pixels at the same d,
// so the gather of the second image's census word touches two or three cache lines per wave for any smooth direction field
// (the mapping epi_rawcost_px_kernel established), and vzInd(d) sits in scalar registers for the whole kernel.  A workgroup
// walks a strip of 64 raw columns (60 output columns + an apron of 2 on either side) down a segment of rows:
//
//   per row y:   raw costs of the 16 d            the reference's fp64 sequence per voxel, 17 instructions
//                horizontal 5-sum, bytes          raw <= 24, so 5 of them fit a byte: the four neighbours' dwords come through
//                                                 a 1 KB per-wave LDS row and add up 4 costs per instruction (v_add3_u32)
//                split to 2 x u16, into a ring    the last five rows' horizontal sums stay in registers (static slots: the
//                                                 row loop is unrolled five times)
//                vertical 5-sum, 2 x u16          sum of 25 raw costs <= 600
//                mean                             (u8)(1.0 * s / 25 + 0.5) == (2 s + 25) / 50 == round(s / 25) (no ties: 25 is
//                                                 odd) == ONE v_pk_mul_f16 by fp16(0.04) on the sums read as denormal fp16
//                                                 patterns: the product of two fp16 values is exact before its single rounding
//                                                 to the denormal grid (= to an integer, nearest-even), and the relative error
//                                                 of fp16(0.04), 2.1e-4, moves s / 25 <= 24 by at most 0.005 -- the nearest tie
//                                                 is 0.02 away.  Checked for every s < 1024 at plan creation (self-test below)
//                                                 and in tests/test_capi_cpu.py.
//                16 bytes of C per lane           the eight waves' stores fill the pixel's 128-byte line between them
//
// Recomputed apron: 64 / 60 columns x (rows + 4) / rows per segment -- 13 % at 64-row segments, 10 % at 125 -- against a
// second kernel that re-reads the raw volume five rows deep (box5x5_sliding16_kernel: 120 MB per 1242x375x128 frame, 0.035 ms).
//
// Rectified form (RECT): Pd0 = (x + 1, y + 1) and direction (-1, 0) or (+1, 0), so the sample of candidate d is
// cen2[y][clamp(x -+ d)] and a strip's samples of one row are a contiguous window of 64 + D - 1 census words (replicate clamp at
// the image edge).  Only the fill differs: per row the workgroup puts that window into LDS once and a lane reads its 16
// consecutive words from there -- no fp64, no gather, no maps, no row_small test.  The window is kept four times, copy c
// shifted by c words, so that a lane whose first word sits at s reads copy s & 3 at the 16-byte aligned word s - (s & 3) as four
// ds_read_b128.  Copies are 16 words (mod 64) apart: the lanes 4 m .. 4 m + 3 of a ds_read_b128 group read one word index in the
// four copies, bank quad m + 4 c, and a group's m values ({0, 3, 5, 6} or {1, 2, 4, 7} mod 8) differ mod 4 -- no conflict.
// The next row's words are requested before this row's tail and written to the other of two LDS rows a step later: one
// workgroup barrier per row.
#include "epi_kernels.h"
#include "fsgm_device.h"
#include <algorithm>

namespace fsgm {

constexpr int CB_OUT = 60;                    // output columns per workgroup (64 raw columns)
constexpr uint32_t CB_K25 = 0x291F291Fu;      // fp16(0.04) twice

// buffer_load_dword ... idxen: address = base + index * stride (stride 4 from the descriptor), so the gather's address is the
// pixel index itself -- one v_mad_u32_u24 per sample instead of a shift and a multiply-add
typedef int cb_i32x4 __attribute__((ext_vector_type(4)));
__device__ uint32_t cb_struct_buffer_load_u32(cb_i32x4 rsrc, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.buffer.load.i32");
__device__ __forceinline__ cb_i32x4 cb_make_rsrc(const void* base, uint32_t records) {
    const uint64_t b = (uint64_t)base;
    cb_i32x4 r;
    r.x = (int)(uint32_t)b;
    r.y = (int)(((uint32_t)(b >> 32) & 0xFFFFu) | (4u << 16));              // stride 4 bytes in bits 61:48
    r.z = (int)records;                                                      // records of `stride` bytes (idxen range check)
    r.w = 0x00020000;                                                        // gfx9 raw dword format
    return r;
}

__device__ __forceinline__ uint32_t pk_mul_f16(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_pk_mul_f16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// one row of a lane's per-pixel operands
struct CbPix {
    double px, py, ux, uy, off;
    uint32_t c1;
};

// a.pd0 / nd / off / vz unused when RECT; rect_dir: -1 / +1, rect_shift: rect_dir * d_min, the columns the window's content lies
// off its place (both RECT only)
template <int NW, bool RECT>
__global__ __launch_bounds__(NW * 64, 4) void epi_costbox_kernel(EpiCostArgs a, uint8_t* __restrict__ Cout, int seg_rows, uint32_t total_items, int rect_dir,
                                                                 int rect_shift) {
    __shared__ __attribute__((aligned(16))) uint4 xch[NW][68];              // a wave's raw row: slots 2 .. 65, two spare either side
    __shared__ __attribute__((aligned(16))) uint4 outt[2][64][NW + 1];      // a row of C, [pixel][16-byte piece], one piece of padding
    constexpr int REACH = 64 + 16 * NW - 1;                                  // RECT: census words a strip's samples of one row span
    constexpr int PITCH = (REACH + 63) / 64 * 64 + 16;                       // words between the shifted copies (16 mod 64)
    constexpr int NPRE = (REACH + NW * 64 - 1) / (NW * 64);                  // words of the window a thread fetches
    __shared__ __attribute__((aligned(16))) uint4 win[RECT ? 2 : 1][RECT ? 4 : 1][RECT ? PITCH / 4 : 1];
    const int W = a.W, H = a.H, D = a.D;
    // Work item of this workgroup.  Workgroups go to the 8 XCDs round-robin by their linear id; the items (strip fastest, then
    // row segment, then frame) are dealt so that every XCD walks a contiguous eighth of the list: the workgroups resident on an
    // XCD then belong to one or two frames and their samples of image 2's census map share that XCD's L2 (with the plain
    // blockIdx order an XCD sees strips of eight frames at once and a scattered direction field fetches 800 MB per frame).
    const int strips = (W + CB_OUT - 1) / CB_OUT, segs = (H + seg_rows - 1) / seg_rows;
    const uint32_t per_xcd = (total_items + 7u) >> 3;
    const uint32_t item = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if ((blockIdx.x >> 3) >= per_xcd || item >= total_items) return;         // uniform over the workgroup
    const int strip = (int)(item % (uint32_t)strips), seg = (int)((item / (uint32_t)strips) % (uint32_t)segs);
    const uint32_t NP = (uint32_t)W * (uint32_t)H;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int d0 = 16 * w;
    const size_t f = item / (uint32_t)(strips * segs);
    const int xs = strip * CB_OUT;
    const int xq = xs - 2 + lane;                      // raw column of this lane (may lie outside: replicate)
    const int px = clampi(xq, 0, W - 1);
    const int y0 = seg * seg_rows, y1 = min(y0 + seg_rows, H);
    const int nsteps = y1 - y0 + 4;                                          // raw rows y0 - 2 .. y1 + 1
    const double* __restrict__ p0 = a.pd0 + f * 2 * (size_t)NP;
    const double* __restrict__ nd = a.nd + f * 2 * (size_t)NP;
    const double* __restrict__ of = a.off + f * (size_t)NP;
    const uint32_t* __restrict__ cen1 = a.cen1 + f * (size_t)NP;
    const char* __restrict__ cen2 = (const char*)(a.cen2 + f * (size_t)NP);
    uint8_t* __restrict__ Cf = Cout + f * (size_t)NP * D;
    const int xhi = W - 1, yhi = H - 1;
    const uint32_t W4 = 4u * (uint32_t)W;                                    // (the general path's byte offsets)
    double vz[16];                                                           // wave-uniform: scalar registers
#pragma unroll
    for (int k = 0; k < 16; k++) vz[k] = RECT ? 0.0 : a.vz[d0 + k];
    const double vzmax = a.vzmax;
    uint4* const myslot = &xch[w][2 + lane];

    auto load_pix = [&](int step) -> CbPix {
        const uint32_t i = (uint32_t)clampi(y0 - 2 + step, 0, yhi) * (uint32_t)W + (uint32_t)px;
        CbPix q;
        if constexpr (RECT) { q.px = q.py = q.ux = q.uy = q.off = 0.0; q.c1 = cen1[i]; }
        else { q.px = p0[i]; q.py = p0[NP + i]; q.ux = nd[i]; q.uy = nd[NP + i]; q.off = of[i]; q.c1 = cen1[i]; }
        return q;
    };
    // The fast rounding (round_clamp_small) differs from x86's (int)round(v) only where v + 0.5 reaches 2^31 (cvttsd2si
    // gives INT_MIN there, which clamps to 0; the GPU's convert saturates to INT_MAX, which clamps to hi); NaN and everything
    // negative clamp to 0 on both sides.  A row whose lanes all keep max(bx, by) + |off| max|vz| max(|ux|, |uy|) below 2^30
    // takes it; any other -- including a NaN in that bound -- takes the restated x86 conversion.
    auto row_small = [&](const CbPix& q) -> bool {
        const double bx = __dsub_rn(q.px, 1.0), by = __dsub_rn(q.py, 1.0);
        const double reach = __dmul_rn(__dmul_rn(fabs(q.off), vzmax), fmax(fabs(q.ux), fabs(q.uy)));
        const bool ok = __dadd_rn(fmax(bx, by), reach) < 1073741824.0;
        return __builtin_amdgcn_ballot_w64(!ok) == 0;
    };
    // byte offsets into image 2's census map of the 8 samples d0 + 8 c + k of this lane's pixel (the reference's sequence)
    auto sample_offsets = [&](const int c, const double bx, const double by, const CbPix& q, uint32_t (&boff)[8]) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double s = __dmul_rn(q.off, vz[8 * c + k]);                                  // offset * vzInd      :360-364
            const double ox = __dmul_rn(s, q.ux), oy = __dmul_rn(s, q.uy);                      // :365-366
            const double vx = __dadd_rn(bx, ox), vy = __dadd_rn(by, oy);
            const int x2 = round_clamp_small(vx, xhi), y2 = round_clamp_small(vy, yhi);         // :371-375
            boff[k] = __umul24((uint32_t)y2, (uint32_t)W) + (uint32_t)x2;                       // pixel index (W < 2^22, H < 2^24: launcher)
        }
    };
    const cb_i32x4 cen2_rsrc = cb_make_rsrc(cen2, NP);
    auto gather = [&](const uint32_t (&idx)[8], uint32_t (&word)[8]) {
#pragma unroll
        for (int k = 0; k < 8; k++) word[k] = cb_struct_buffer_load_u32(cen2_rsrc, (int)idx[k], 0, 0, 0);
    };
    auto hamming = [&](const uint32_t c1, const uint32_t (&word)[8], uint32_t& lo, uint32_t& hi) {
        uint32_t c[8];
#pragma unroll
        for (int k = 0; k < 8; k++) c[k] = __popc(c1 ^ word[k]);                                // :377-378
        auto pack4 = [](uint32_t c0, uint32_t c1_, uint32_t c2, uint32_t c3) {
            uint32_t t, u, r;
            asm("v_lshl_or_b32 %0, %1, 8, %2" : "=v"(t) : "v"(c1_), "v"(c0));
            asm("v_lshl_or_b32 %0, %1, 8, %2" : "=v"(u) : "v"(c3), "v"(c2));
            asm("v_lshl_or_b32 %0, %1, 16, %2" : "=v"(r) : "v"(u), "v"(t));
            return r;
        };
        lo = pack4(c[0], c[1], c[2], c[3]); hi = pack4(c[4], c[5], c[6], c[7]);
    };

    uint32_t ring[5][8];                                                     // horizontal 5-sums of the last five rows, 2 x u16
#pragma unroll
    for (int s = 0; s < 5; s++)
#pragma unroll
        for (int i = 0; i < 8; i++) ring[s][i] = 0;

    // A step = the fill of raw row `st` (st < nsteps) with the tail of row st - 1 tucked between the gathers' issue and their
    // use: horizontal sums through LDS, ring update, vertical sum, mean, store of output row y0 + st - 5.  Software pipeline:
    // the next row's operands are requested once this row's offsets are out and used a step later; no register double-buffering.
    CbPix cur = load_pix(0);
    uint4 raw = make_uint4(0, 0, 0, 0);

    auto tail = [&](const int st, uint32_t (&slot)[8]) {                     // raw = costs of raw row st
        // horizontal 5-sum across the lanes, in bytes (<= 120)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        *myslot = raw;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint4 m2 = myslot[-2], m1 = myslot[-1], p1 = myslot[1], p2 = myslot[2];
        __builtin_amdgcn_wave_barrier();
        const uint32_t h[4] = {raw.x + m2.x + m1.x + p1.x + p2.x, raw.y + m2.y + m1.y + p1.y + p2.y,
                               raw.z + m2.z + m1.z + p1.z + p2.z, raw.w + m2.w + m1.w + p1.w + p2.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            slot[2 * i] = h[i] & 0x00FF00FFu;                                // d = 4 i, 4 i + 2
            slot[2 * i + 1] = __builtin_amdgcn_perm(0u, h[i], 0x0C030C01u);  // d = 4 i + 1, 4 i + 3
        }
        const int yo = y0 + st - 4;                                          // the row whose five raw rows are now in the ring
        if (st >= 4) {                                                       // wave-uniform
            uint32_t o[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t se = ring[0][2 * i] + ring[1][2 * i] + ring[2][2 * i] + ring[3][2 * i] + ring[4][2 * i];
                const uint32_t so = ring[0][2 * i + 1] + ring[1][2 * i + 1] + ring[2][2 * i + 1] + ring[3][2 * i + 1] + ring[4][2 * i + 1];
                const uint32_t me = pk_mul_f16(se, CB_K25), mo = pk_mul_f16(so, CB_K25);   // :403-404
                asm("v_lshl_or_b32 %0, %1, 8, %2" : "=v"(o[i]) : "v"(mo), "v"(me));
            }
            // the waves' 16-byte pieces of a pixel meet in LDS and leave as whole lines: wave w stores pixels 64 / NW * w ...,
            // one 16-byte piece per lane (16-byte stores 128 bytes apart were measured at 1.85 x the written bytes in HBM)
            outt[st & 1][lane][w] = make_uint4(o[0], o[1], o[2], o[3]);
        }
        if (st >= 4) {
            __syncthreads();                                                 // every wave runs the same steps: uniform
            constexpr int PPW = 64 / NW;                                     // pixels a wave stores
            const int pl = w * PPW + lane / NW, piece = lane % NW;           // pixel (= lane of the producers), piece
            const int xo = xs - 2 + pl;
            if (pl >= 2 && pl < 2 + CB_OUT && xo < W)
                *(uint4*)(Cf + ((uint32_t)yo * (uint32_t)W + (uint32_t)xo) * (uint32_t)D + 16u * piece) = outt[st & 1][pl][piece];
        }
    };
    auto fill_general = [&](const int st, uint32_t (&pslot)[8]) {
        if (st >= 1) tail(st - 1, pslot);                                    // wave-uniform
        const double bx = __dsub_rn(cur.px, 1.0), by = __dsub_rn(cur.py, 1.0);
        const double* vzp = a.vz + d0;
#pragma clang loop unroll(disable)
        for (int k = 0; k < 16; k++) {
            const double s = __dmul_rn(cur.off, vzp[k]);
            const double ox = __dmul_rn(s, cur.ux), oy = __dmul_rn(s, cur.uy);
            const int x2 = clamp0(round_to_i32_x86(__dadd_rn(bx, ox)), xhi), y2 = clamp0(round_to_i32_x86(__dadd_rn(by, oy)), yhi);
            const uint32_t cost = __popc(cur.c1 ^ *(const uint32_t*)(cen2 + (__umul24((uint32_t)y2, W4) + ((uint32_t)x2 << 2))));
            raw.x = __builtin_amdgcn_alignbit(raw.y, raw.x, 8);              // the 16 bytes as one shift register: byte k enters at the top
            raw.y = __builtin_amdgcn_alignbit(raw.z, raw.y, 8);
            raw.z = __builtin_amdgcn_alignbit(raw.w, raw.z, 8);
            raw.w = (raw.w >> 8) | (cost << 24);
        }
        cur = load_pix(min(st + 1, nsteps - 1));
    };
    // xonly: every lane of the row has a direction with uy == 0 (horizontal epipolar lines: a rectified pair, the survey's
    // timing maps) -- offset * vzInd * 0 is a zero of either sign for the finite products a small row has, by + (+-0) is by,
    // so the sample row is round(by) for every d (:372, :375) and only the x coordinate walks: 11 instructions a voxel, not 17.
    // (A wave-uniform branch around the two forms of the offsets only: a third copy of the whole step cost the register
    // allocation 54 spills.)
    auto sample_offsets_x = [&](const int c, const double bx, const uint32_t rowoff, const CbPix& q, uint32_t (&boff)[8]) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double s = __dmul_rn(q.off, vz[8 * c + k]);
            const double vx = __dadd_rn(bx, __dmul_rn(s, q.ux));
            boff[k] = rowoff + (uint32_t)round_clamp_small(vx, xhi);
        }
    };
    auto fill = [&](const int st, uint32_t (&pslot)[8]) {
        const double bx = __dsub_rn(cur.px, 1.0), by = __dsub_rn(cur.py, 1.0);                 // :348-349
        const bool xonly = __builtin_amdgcn_ballot_w64(cur.uy != 0.0) == 0;                    // (+-0 compare equal to 0; NaN does not)
        const uint32_t rowoff = __umul24((uint32_t)round_clamp_small(by, yhi), (uint32_t)W);
        uint32_t w0[8], w1[8];
        if (xonly) sample_offsets_x(0, bx, rowoff, cur, w0); else sample_offsets(0, bx, by, cur, w0);
        gather(w0, w0);
        if (xonly) sample_offsets_x(1, bx, rowoff, cur, w1); else sample_offsets(1, bx, by, cur, w1);
        gather(w1, w1);
        const uint32_t c1 = cur.c1;
        cur = load_pix(min(st + 1, nsteps - 1));                             // (past the last row: the last row again, never used)
        if (st >= 1) tail(st - 1, pslot);                                    // wave-uniform
        hamming(c1, w0, raw.x, raw.y);
        hamming(c1, w1, raw.z, raw.w);
    };

    // ---- RECT: the window of image 2's census row.  xb: the image column of window word 0; the lane's pixel px (its raw
    // column, clamped) samples words (px - xb) + dir * d, all inside [0, REACH): see the launcher's comment.  A search range that
    // starts at d_min moves what the words HOLD, never which word a lane reads: word i is image column xb + rect_shift + i,
    // clamped at either image edge by the fill (xc: that column of word 0; |rect_shift| <= 1024, the sum stays far inside int) ----
    const int xb = rect_dir < 0 ? xs - 2 - (16 * NW - 1) : xs - 2;
    const int xc = xb + rect_shift;
    const int s0w = rect_dir < 0 ? px - xb - d0 - 15 : px - xb + d0;         // the lowest of the lane's 16 window words
    const int wc = s0w & 3, wq = s0w >> 2;                                   // its copy and 16-byte slot there
    uint32_t pre[NPRE];
    auto load_window = [&](int step) {
        const uint32_t* row = (const uint32_t*)cen2 + (uint32_t)clampi(y0 - 2 + step, 0, yhi) * (uint32_t)W;
#pragma unroll
        for (int n = 0; n < NPRE; n++) {
            const int i = (int)threadIdx.x + n * NW * 64;
            pre[n] = i < REACH ? row[clampi(xc + i, 0, xhi)] : 0u;
        }
    };
    auto fill_rect = [&](const int st, uint32_t (&pslot)[8]) {
        uint32_t* const wrow = (uint32_t*)&win[st & 1][0][0];
#pragma unroll
        for (int n = 0; n < NPRE; n++) {
            const int i = (int)threadIdx.x + n * NW * 64;
            if (i < REACH) {
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if (i >= c) wrow[c * PITCH + i - c] = pre[n];            // copy c: word j = window word j + c
            }
        }
        const uint32_t c1 = cur.c1;
        load_window(min(st + 1, nsteps - 1));
        cur = load_pix(min(st + 1, nsteps - 1));
        __syncthreads();                                                     // every wave runs the same steps: uniform
        const uint4* const wp = &win[st & 1][wc][wq];
        const uint4 q0 = wp[0], q1 = wp[1], q2 = wp[2], q3 = wp[3];
        if (st >= 1) tail(st - 1, pslot);                                    // wave-uniform
        const uint32_t wd[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
        uint32_t up[8], dn[8];                                               // window words in ascending order = d ascending (+1) or descending (-1)
        if (rect_dir < 0) {                                                  // uniform
#pragma unroll
            for (int k = 0; k < 8; k++) { up[k] = wd[15 - k]; dn[k] = wd[7 - k]; }
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) { up[k] = wd[k]; dn[k] = wd[8 + k]; }
        }
        hamming(c1, up, raw.x, raw.y);
        hamming(c1, dn, raw.z, raw.w);
    };

    if constexpr (RECT) load_window(0);
    for (int base = 0; base < nsteps; base += 5) {
#pragma unroll
        for (int k = 0; k < 5; k++)
            if (base + k < nsteps) {                                         // wave-uniform
                if constexpr (RECT) fill_rect(base + k, ring[(k + 4) % 5]);
                else if (row_small(cur)) fill(base + k, ring[(k + 4) % 5]);
                else                     fill_general(base + k, ring[(k + 4) % 5]);
            }
    }
    // the last raw row's tail
    switch ((nsteps - 1) % 5) {
        case 0: tail(nsteps - 1, ring[0]); break;
        case 1: tail(nsteps - 1, ring[1]); break;
        case 2: tail(nsteps - 1, ring[2]); break;
        case 3: tail(nsteps - 1, ring[3]); break;
        default: tail(nsteps - 1, ring[4]); break;
    }
}

// self-test of the mean's multiply (every sum a 5x5 window of census costs can reach, and beyond): 0 = exact
__global__ void costbox_selftest_kernel(uint32_t* bad) {
    const uint32_t s = threadIdx.x + 256u * blockIdx.x;                      // 0 .. 1023
    const uint32_t got = pk_mul_f16(s | (s << 16), CB_K25);
    const uint32_t want = (2 * s + 25) / 50;
    if ((got & 0xFFFFu) != want || (got >> 16) != want) atomicAdd(bad, 1u);
}

int costbox_selftest(hipStream_t st) {
    uint32_t* d = nullptr;
    uint32_t h = 1;
    if (hipMalloc((void**)&d, 4) != hipSuccess) return -1;
    bool ok = hipMemsetAsync(d, 0, 4, st) == hipSuccess;
    if (ok) hipLaunchKernelGGL(costbox_selftest_kernel, dim3(4), dim3(256), 0, st, d);
    ok = ok && hipMemcpyAsync(&h, d, 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    (void)hipFree(d);
    return ok ? (int)h : -1;
}

bool costbox_ok(int W, int H, int D) {
    return (D == 16 || D == 32 || D == 64 || D == 128 || D == 256) && W < (1 << 22) && H < (1 << 24);
}

// Rows per segment.  A workgroup's time goes with its rows + 4 (the apron rows), the launch's with the rounds of resident
// workgroups it takes (16 waves per CU at <= 128 VGPRs: 16 / NW workgroups): the segment count that minimises
// rounds x (rows + 4) -- few long segments once the frames alone fill the chip, many short ones for a single frame.
int costbox_seg_rows(int W, int H, int D, int frames, int cus) {
    const long long strips = (W + CB_OUT - 1) / CB_OUT;
    const long long resident = (long long)cus * std::max(1, 16 / (D >> 4));
    long long best = -1;
    int best_rows = H;
    for (int nseg = 1; nseg <= std::max(1, H / 8); nseg++) {
        const int rows = (H + nseg - 1) / nseg;                              // equal segments: 375 rows -> 3 x 125, not 128 + 128 + 119
        const long long items = strips * ((H + rows - 1) / rows) * frames;
        const long long cost = ((items + resident - 1) / resident) * (rows + 4);
        if (best < 0 || cost < best) { best = cost; best_rows = rows; }
    }
    return best_rows;
}

static void launch_costbox(hipStream_t st, const EpiCostArgs& a, uint8_t* C, int frames, int rect_dir, int rect_shift = 0) {
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        return n;
    }();
    const int seg = costbox_seg_rows(a.W, a.H, a.D, frames, cus);
    const uint32_t total = (uint32_t)((a.W + CB_OUT - 1) / CB_OUT) * (uint32_t)((a.H + seg - 1) / seg) * (uint32_t)frames;
    dim3 grid(8u * ((total + 7u) / 8u));
    if (rect_dir == 0) {
        switch (a.D >> 4) {
#define FSGM_CB(NW) case NW: hipLaunchKernelGGL((epi_costbox_kernel<NW, false>), grid, dim3(NW * 64), 0, st, a, C, seg, total, 0, 0); break;
            FSGM_CB(1) FSGM_CB(2) FSGM_CB(4) FSGM_CB(8) FSGM_CB(16)
#undef FSGM_CB
        }
    } else {
        switch (a.D >> 4) {
#define FSGM_CB(NW) case NW: hipLaunchKernelGGL((epi_costbox_kernel<NW, true>), grid, dim3(NW * 64), 0, st, a, C, seg, total, rect_dir, rect_shift); break;
            FSGM_CB(1) FSGM_CB(2) FSGM_CB(4) FSGM_CB(8) FSGM_CB(16)
#undef FSGM_CB
        }
    }
}

void launch_epi_costbox(hipStream_t st, const EpiCostArgs& a, uint8_t* C, int frames) { launch_costbox(st, a, C, frames, 0); }

// =============================================================================================
// The two-kernel form: raw Hamming cost along the epipolar line  (calc_cost_sgm.cpp:343-381) into a raw volume in HBM.
// One thread = one pixel x 4 consecutive d.  fp64 geometry in the reference's association
// order with explicit round-to-nearest mul/add (no FMA contraction).
// =============================================================================================
template <bool VEC4>                                       // VEC4: D % 4 == 0, no per-element guards, one u32 store
__global__ __launch_bounds__(256) void epi_rawcost_kernel(EpiCostArgs a) {
    const int W = a.W, H = a.H, D = a.D;
    const int NP = W * H;
    const int Dq = (D + 3) >> 2;
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;        // NP * Dq < 2^31 (checked on the host)
    if (gid >= (uint32_t)NP * (uint32_t)Dq) return;
    const int p = (int)(gid / (uint32_t)Dq), q = (int)(gid - (uint32_t)p * (uint32_t)Dq);
    const size_t f = blockIdx.y;
    const double* __restrict__ p0 = a.pd0 + f * 2 * (size_t)NP;
    const double* __restrict__ nd = a.nd + f * 2 * (size_t)NP;
    const double bx = __dsub_rn(p0[p], 1.0), by = __dsub_rn(p0[NP + p], 1.0);          // :348-349
    const double ux = nd[p], uy = nd[NP + p];
    const double off = a.off[f * (size_t)NP + p];
    const uint32_t* __restrict__ cen2 = a.cen2 + f * (size_t)NP;
    const uint32_t c1 = a.cen1[f * (size_t)NP + p];
    uint8_t* out = a.Craw + f * (size_t)NP * D + (uint32_t)p * (uint32_t)D + 4u * q;
    const double* __restrict__ vz = a.vz + 4 * q;
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (VEC4 || 4 * q + k < D) {
            const double s = __dmul_rn(off, vz[k]);                                        // offset * vzInd
            const double ox = __dmul_rn(s, ux), oy = __dmul_rn(s, uy);                    // :365-366
            int x2 = round_to_i32_x86(__dadd_rn(bx, ox));                                 // :371
            int y2 = round_to_i32_x86(__dadd_rn(by, oy));                                 // :372
            x2 = clampi(x2, 0, W - 1);
            y2 = clampi(y2, 0, H - 1);
            const uint32_t cost = __popc(c1 ^ cen2[y2 * W + x2]);                         // :377-378
            packed |= cost << (8 * k);
        }
    }
    if (VEC4) {
        *(uint32_t*)out = packed;
    } else {
        for (int k = 0; k < 4; k++)
            if (4 * q + k < D) out[k] = (uint8_t)(packed >> (8 * k));
    }
}

// Same for D % 8 == 0, one thread = one pixel, all d.  Neighbouring lanes are neighbouring pixels at the
// same d, so the gather of the second image's census word touches two or three cache lines per wave
// whatever the direction of the epipolar lines (with d across lanes every lane lands in its own line and
// the kernel is bound by the L1 tag rate); vzInd(d) is wave-uniform and comes from scalar loads; the
// per-pixel maps are read once, coalesced.  The 8 costs of a chunk are packed and parked in a per-wave
// LDS tile [64 px][128 B + 8 pad] and written out as full 128-B lines.  ~30 VALU instructions per voxel,
// most of them the reference's own fp64 sequence (3 mul, 2 add, 2 x round-half-away + truncate).
// SMALL: every sample position of the wave is below 2^30 in magnitude (checked per pixel from the maps and
// max |vzInd|), so the rounding needs no range test.
constexpr int RC_SEG = 128, RC_PAD = RC_SEG + 8;
template <bool SMALL>
__device__ __forceinline__ void epi_rawcost_px_body(const EpiCostArgs& a, uint8_t* tilew, const uint32_t pw, const uint32_t p,
                                                    const double bx, const double by, const double ux, const double uy, const double off) {
    const int W = a.W, H = a.H, D = a.D;
    const uint32_t NP = (uint32_t)W * (uint32_t)H;
    const int lane = threadIdx.x & 63;
    const size_t f = blockIdx.y;
    const char* __restrict__ cen2 = (const char*)(a.cen2 + f * (size_t)NP);
    const uint32_t c1 = a.cen1[f * (size_t)NP + p];
    const double* __restrict__ vzt = a.vz;
    const int xhi = W - 1, yhi = H - 1;
    const uint32_t W4 = 4u * (uint32_t)W;
    uint8_t* const myrow = tilew + lane * RC_PAD;
    uint8_t* const outw = a.Craw + f * (size_t)NP * D + (size_t)pw * D;
    // byte offsets of the 8 census words chunk (d0 + c) of this pixel samples: the reference's fp64 sequence per voxel
    auto sample_offsets = [&](const int dbase, uint32_t (&boff)[8]) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double s = __dmul_rn(off, vzt[dbase + k]);                                  // offset * vzInd
            const double ox = __dmul_rn(s, ux), oy = __dmul_rn(s, uy);                        // :365-366
            const double vx = __dadd_rn(bx, ox), vy = __dadd_rn(by, oy);
            const int x2 = SMALL ? round_clamp_small(vx, xhi) : clamp0(round_to_i32_x86(vx), xhi);   // :371, :374
            const int y2 = SMALL ? round_clamp_small(vy, yhi) : clamp0(round_to_i32_x86(vy), yhi);   // :372, :375
            boff[k] = __umul24((uint32_t)y2, W4) + ((uint32_t)x2 << 2);                       // 4W, H < 2^24 (launcher)
        }
    };
    for (int d0 = 0; d0 < D; d0 += RC_SEG) {
        const int sb = min(RC_SEG, D - d0);
        // Software pipeline over the chunks of 8 d: the gathered census words of chunk c are requested before the
        // arithmetic of chunk c+1 (some 200 instructions) and consumed after it, so the gather's latency -- L2 hits, a
        // few hundred cycles -- no longer parks the wave once per chunk (round 3 counters: 29 % of the wave time in
        // s_waitcnt with the loads waited for where they were issued).
        uint32_t boff[8], word[8];
        sample_offsets(d0, boff);
#pragma unroll
        for (int k = 0; k < 8; k++) word[k] = *(const uint32_t*)(cen2 + boff[k]);
        for (int c = 0; c < sb; c += 8) {
            uint32_t nword[8];
            if (c + 8 < sb) {                                                                 // wave-uniform
                sample_offsets(d0 + c + 8, boff);
#pragma unroll
                for (int k = 0; k < 8; k++) nword[k] = *(const uint32_t*)(cen2 + boff[k]);
            }
            uint32_t packed[2] = {0, 0};
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t cost = __popc(c1 ^ word[k]);                                   // :377-378
                asm("v_lshl_or_b32 %0, %1, %2, %0" : "+v"(packed[k >> 2]) : "v"(cost), "n"(8 * (k & 3)));
            }
            *(uint2*)(myrow + c) = make_uint2(packed[0], packed[1]);
#pragma unroll
            for (int k = 0; k < 8; k++) word[k] = nword[k];
        }
        __builtin_amdgcn_wave_barrier();
        for (uint32_t e = lane * 8u; e < 64u * (uint32_t)sb; e += 512u) {                     // tile -> HBM, whole lines
            const uint32_t px = e / (uint32_t)sb, o = e - px * (uint32_t)sb;
            if (pw + px < NP) *(uint2*)(outw + (size_t)px * D + d0 + o) = *(const uint2*)(tilew + px * RC_PAD + o);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ __launch_bounds__(256) void epi_rawcost_px_kernel(EpiCostArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[4][64 * RC_PAD];
    const uint32_t NP = (uint32_t)a.W * (uint32_t)a.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t pw = (blockIdx.x * 4u + wave) * 64u;          // first pixel of this wave
    if (pw >= NP) return;                                        // wave-uniform
    const uint32_t p = min(pw + lane, NP - 1);                   // lanes past the end redo the last pixel, never stored
    const size_t f = blockIdx.y;
    const double* __restrict__ p0 = a.pd0 + f * 2 * (size_t)NP;
    const double* __restrict__ nd = a.nd + f * 2 * (size_t)NP;
    const double bx = __dsub_rn(p0[p], 1.0), by = __dsub_rn(p0[NP + p], 1.0);          // :348-349
    const double ux = nd[p], uy = nd[NP + p];
    const double off = a.off[f * (size_t)NP + p];
    // |off * vz * u| <= reach * (1 + 3 ulp); NaN or inf anywhere fails the compares
    const double reach = __dmul_rn(__dmul_rn(fabs(off), a.vzmax), fmax(fabs(ux), fabs(uy)));
    const bool small = fabs(bx) < 536870912.0 && fabs(by) < 536870912.0 && reach < 536870912.0 &&
                       fabs(ux) <= 1.7e308 && fabs(uy) <= 1.7e308;
    if (__builtin_amdgcn_ballot_w64(!small) == 0) epi_rawcost_px_body<true>(a, tile[wave], pw, p, bx, by, ux, uy, off);
    else                                          epi_rawcost_px_body<false>(a, tile[wave], pw, p, bx, by, ux, uy, off);
}

// =============================================================================================
// 5x5 box mean, replicate border  (calc_cost_sgm.cpp:387-407).
// (u8)(1.0*sum/25 + 0.5) == (2*sum + 25) / 50 in integers: the exact value has denominator 50,
// so it is never within 1/50 of an integer from below except at the integer itself, which
// needs 2*sum+25 (odd) divisible by 50 -- impossible.
// One thread = one pixel x 4 consecutive d (SWAR: even/odd bytes summed in 16-bit fields).
// =============================================================================================
__global__ __launch_bounds__(256) void box5x5_kernel(const uint8_t* __restrict__ Craw,
                                                     uint8_t* __restrict__ C, int W, int H, int D) {
    const int NP = W * H;
    const int Dq = (D + 3) >> 2;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)NP * Dq) return;
    const int p = (int)(gid / Dq), q = (int)(gid - (long long)p * Dq);
    const int y = p / W, x = p - y * W;
    const uint8_t* raw = Craw + (size_t)blockIdx.y * NP * D;
    uint8_t* out = C + (size_t)blockIdx.y * NP * D + (size_t)p * D + 4 * q;
    if ((D & 3) == 0) {
        uint32_t se = 0, so = 0;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const int y1 = clampi(y + dy, 0, H - 1);
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int x1 = clampi(x + dx, 0, W - 1);
                const uint32_t w = *(const uint32_t*)(raw + ((size_t)y1 * W + x1) * D + 4 * q);
                se += w & 0x00FF00FFu;
                so += (w >> 8) & 0x00FF00FFu;
            }
        }
        const uint32_t b0 = (2 * (se & 0xFFFF) + 25) / 50, b2 = (2 * (se >> 16) + 25) / 50;
        const uint32_t b1 = (2 * (so & 0xFFFF) + 25) / 50, b3 = (2 * (so >> 16) + 25) / 50;
        *(uint32_t*)out = (b0 & 0xFF) | ((b1 & 0xFF) << 8) | ((b2 & 0xFF) << 16) | ((b3 & 0xFF) << 24);
    } else {
        for (int k = 0; k < 4; k++) {
            const int d = 4 * q + k;
            if (d >= D) break;
            uint32_t s = 0;
            for (int dy = -2; dy <= 2; dy++) {
                const int y1 = clampi(y + dy, 0, H - 1);
                for (int dx = -2; dx <= 2; dx++) {
                    const int x1 = clampi(x + dx, 0, W - 1);
                    s += raw[((size_t)y1 * W + x1) * D + d];
                }
            }
            out[k] = (uint8_t)((2 * s + 25) / 50);
        }
    }
}

// =============================================================================================
// 5x5 box mean, sliding-window form for D % 4 == 0 (same result as box5x5_kernel).
// One thread = one pixel column x 4 consecutive d, walking down BOX_ROWS rows: per row one
// horizontal 5-sum (5 u32 loads, even/odd bytes in 16-bit fields) and a 5-deep ring of those sums
// for the vertical part: 5 loads per output instead of 25.
// =============================================================================================
constexpr int BOX_ROWS = 32;
__global__ __launch_bounds__(256) void box5x5_sliding_kernel(const uint8_t* __restrict__ Craw,
                                                             uint8_t* __restrict__ C, int W, int H, int D) {
    const int Dq = D >> 2;
    const int cols = 256 / Dq;                               // pixel columns per block (Dq <= 256 here)
    const int q = threadIdx.x % Dq, xi = threadIdx.x / Dq;
    const int x = blockIdx.x * cols + xi;
    if (xi >= cols || x >= W) return;
    const int y0 = blockIdx.y * BOX_ROWS, y1 = min(y0 + BOX_ROWS, H);
    const size_t NP = (size_t)W * H;
    const uint8_t* raw = Craw + (size_t)blockIdx.z * NP * D + 4 * q;
    uint8_t* out = C + (size_t)blockIdx.z * NP * D + 4 * q;
    int xs[5];
#pragma unroll
    for (int k = 0; k < 5; k++) xs[k] = clampi(x + k - 2, 0, W - 1);
    auto hsum = [&](int y, uint32_t& he, uint32_t& ho) {     // horizontal 5-sum of row clamp(y)
        const uint8_t* r = raw + (size_t)clampi(y, 0, H - 1) * W * D;
        he = 0; ho = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const uint32_t w = *(const uint32_t*)(r + (size_t)xs[k] * D);
            he += w & 0x00FF00FFu;
            ho += (w >> 8) & 0x00FF00FFu;
        }
    };
    uint32_t re[5], ro[5];                                   // ring: rows y-2 .. y+2 around the output row
#pragma unroll
    for (int k = 0; k < 4; k++) hsum(y0 - 2 + k, re[k], ro[k]);
    for (int yb = y0; yb < y1; yb += 5) {
#pragma unroll
        for (int k = 0; k < 5; k++) {                        // static ring slot = (k + 4) % 5
            const int y = yb + k;
            if (y < y1) {
                hsum(y + 2, re[(k + 4) % 5], ro[(k + 4) % 5]);
                const uint32_t se = re[0] + re[1] + re[2] + re[3] + re[4];
                const uint32_t so = ro[0] + ro[1] + ro[2] + ro[3] + ro[4];
                const uint32_t b0 = (2 * (se & 0xFFFF) + 25) / 50, b2 = (2 * (se >> 16) + 25) / 50;
                const uint32_t b1 = (2 * (so & 0xFFFF) + 25) / 50, b3 = (2 * (so >> 16) + 25) / 50;
                *(uint32_t*)(out + ((size_t)y * W + x) * D) = (b0 & 0xFF) | ((b1 & 0xFF) << 8) | ((b2 & 0xFF) << 16) | ((b3 & 0xFF) << 24);
            }
        }
    }
}

// =============================================================================================
// The same sliding window with 16 bytes per lane (D % 16 == 0): one thread = one pixel column x 16 consecutive d, D/16
// adjacent lanes a pixel -- every access a 16-byte one, a wave's load 64/(D/16) whole pixels (the dword form above moves
// 4 bytes a lane and reaches 3.5 TB/s; 16-byte accesses are what this chip's memory pipeline is built for).
// =============================================================================================
__global__ __launch_bounds__(256) void box5x5_sliding16_kernel(const uint8_t* __restrict__ Craw,
                                                               uint8_t* __restrict__ C, int W, int H, int D) {
    const int Dq = D >> 4;                                   // lanes per pixel
    const int cols = 256 / Dq;                               // pixel columns per block (Dq <= 64 here)
    const int q = threadIdx.x % Dq, xi = threadIdx.x / Dq;
    const int x = blockIdx.x * cols + xi;
    if (xi >= cols || x >= W) return;
    const int y0 = blockIdx.y * BOX_ROWS, y1 = min(y0 + BOX_ROWS, H);
    const size_t NP = (size_t)W * H;
    const uint8_t* raw = Craw + (size_t)blockIdx.z * NP * D + 16 * q;
    uint8_t* out = C + (size_t)blockIdx.z * NP * D + 16 * q;
    uint32_t xo[5];
#pragma unroll
    for (int k = 0; k < 5; k++) xo[k] = (uint32_t)clampi(x + k - 2, 0, W - 1) * (uint32_t)D;
    struct Sum { uint32_t e[4], o[4]; };                     // even / odd bytes of the 4 dwords in 16-bit fields
    auto hsum = [&](int y, Sum& h) {                         // horizontal 5-sum of row clamp(y)
        const uint8_t* r = raw + (size_t)clampi(y, 0, H - 1) * W * D;
#pragma unroll
        for (int i = 0; i < 4; i++) { h.e[i] = 0; h.o[i] = 0; }
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const uint4 v = *(const uint4*)(r + xo[k]);       // neighbouring lanes re-read these lines: through the L1
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; i++) { h.e[i] += w[i] & 0x00FF00FFu; h.o[i] += (w[i] >> 8) & 0x00FF00FFu; }
        }
    };
    Sum ring[5];                                             // rows y-2 .. y+2 around the output row
#pragma unroll
    for (int k = 0; k < 4; k++) hsum(y0 - 2 + k, ring[k]);
    for (int yb = y0; yb < y1; yb += 5) {
#pragma unroll
        for (int k = 0; k < 5; k++) {                        // static ring slot = (k + 4) % 5
            const int y = yb + k;
            if (y < y1) {
                hsum(y + 2, ring[(k + 4) % 5]);
                uint32_t o4[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t se = ring[0].e[i] + ring[1].e[i] + ring[2].e[i] + ring[3].e[i] + ring[4].e[i];
                    const uint32_t so = ring[0].o[i] + ring[1].o[i] + ring[2].o[i] + ring[3].o[i] + ring[4].o[i];
                    const uint32_t b0 = (2 * (se & 0xFFFF) + 25) / 50, b2 = (2 * (se >> 16) + 25) / 50;
                    const uint32_t b1 = (2 * (so & 0xFFFF) + 25) / 50, b3 = (2 * (so >> 16) + 25) / 50;
                    o4[i] = (b0 & 0xFF) | ((b1 & 0xFF) << 8) | ((b2 & 0xFF) << 16) | ((b3 & 0xFF) << 24);
                }
                *(uint4*)(out + ((size_t)y * W + x) * D) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
            }
        }
    }
}

// ---- which kernels the cost stage runs (the launchers here switch on this; fsgm_epi_cost_kernels prints it) ----
int select_box_kernel(int D) {
    static const bool box16 = [] { const char* e = getenv("FSGM_BOX16"); return !(e && e[0] == '0'); }();   // A/B switch
    if (box16 && (D & 15) == 0 && D <= 1024) return COST_BOX_16;            // D / 16 <= 64 lanes a pixel
    if ((D & 3) == 0 && D <= 1024) return COST_BOX_4;                        // D / 4 <= 256 lanes a pixel
    return COST_BOX_1;
}

CostKernels select_cost_kernels(int W, int H, int D, bool rectified) {
    // FSGM_COST_FUSED=0: the two-kernel form (raw volume through HBM) -- A/B switch and the cross-check of the fused kernel in the tests
    const bool fused = [] { const char* e = getenv("FSGM_COST_FUSED"); return !(e && e[0] == '0'); }();   // read per call: the tests flip it
    if (fused && costbox_ok(W, H, D)) return {COST_RAW_FUSED, COST_BOX_FUSED};
    int raw;
    if (rectified) raw = COST_RAW_STEREO;
    else if ((D & 7) == 0 && W < (1 << 22) && H < (1 << 24)) raw = COST_RAW_PX;   // (the px kernel's 24-bit multiplies)
    else if ((D & 3) == 0) raw = COST_RAW_VEC4;
    else raw = COST_RAW_SCALAR;
    return {raw, select_box_kernel(D)};
}

const char* cost_kernels_name(CostKernels k, bool rectified) {
    static const char* const names[5][4] = {{"costbox", "", "", ""},
                                            {"", "px+box16", "px+box4", "px+box1"},
                                            {"", "vec4+box16", "vec4+box4", "vec4+box1"},
                                            {"", "scalar+box16", "scalar+box4", "scalar+box1"},
                                            {"", "stereo+box16", "stereo+box4", "stereo+box1"}};
    if (k.raw == COST_RAW_FUSED) return rectified ? "stereo-costbox" : "costbox";
    return names[k.raw][k.box];
}

void launch_epi_cost(hipStream_t st, const EpiCostArgs& a, uint8_t* C, int frames) {
    const CostKernels k = select_cost_kernels(a.W, a.H, a.D, false);
    const long long n = (long long)a.W * a.H * ((a.D + 3) / 4);
    dim3 grid((unsigned)((n + 255) / 256), frames);
    switch (k.raw) {
        case COST_RAW_FUSED: launch_epi_costbox(st, a, C, frames); return;
        case COST_RAW_PX:
            hipLaunchKernelGGL(epi_rawcost_px_kernel, dim3((unsigned)(((long long)a.W * a.H + 255) / 256), frames), dim3(256), 0, st, a);
            break;
        case COST_RAW_VEC4: hipLaunchKernelGGL(epi_rawcost_kernel<true>, grid, dim3(256), 0, st, a); break;
        default:            hipLaunchKernelGGL(epi_rawcost_kernel<false>, grid, dim3(256), 0, st, a); break;
    }
    launch_box5x5(st, k.box, a.Craw, C, a.W, a.H, a.D, frames);
}

// the 5x5 box mean of a raw volume in HBM (the two-kernel form of the cost stage); box: select_box_kernel(D)
void launch_box5x5(hipStream_t st, int box, const uint8_t* Craw, uint8_t* C, int W, int H, int D, int frames) {
    switch (box) {
        case COST_BOX_16: {
            const int cols = 256 / (D >> 4);
            dim3 g2((W + cols - 1) / cols, (H + BOX_ROWS - 1) / BOX_ROWS, frames);
            hipLaunchKernelGGL(box5x5_sliding16_kernel, g2, dim3(256), 0, st, Craw, C, W, H, D);
            break;
        }
        case COST_BOX_4: {
            const int cols = 256 / (D >> 2);
            dim3 g2((W + cols - 1) / cols, (H + BOX_ROWS - 1) / BOX_ROWS, frames);
            hipLaunchKernelGGL(box5x5_sliding_kernel, g2, dim3(256), 0, st, Craw, C, W, H, D);
            break;
        }
        default: {
            const long long n = (long long)W * H * ((D + 3) / 4);
            hipLaunchKernelGGL(box5x5_kernel, dim3((unsigned)((n + 255) / 256), frames), dim3(256), 0, st, Craw, C, W, H, D);
            break;
        }
    }
}

// Rectified pair, any dMax: raw costs of one (pixel, d) per thread into the raw volume for the box kernels; index d stands for
// disparity d_min + d
__global__ __launch_bounds__(256) void stereo_rawcost_kernel(const uint32_t* __restrict__ cen1, const uint32_t* __restrict__ cen2,
                                                             uint8_t* __restrict__ Craw, int W, int H, int D, int dir, int d_min) {
    const size_t NP = (size_t)W * H;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= NP * D) return;
    const uint32_t p = (uint32_t)(gid / D), d = (uint32_t)(gid - (size_t)p * D);
    const int y = (int)(p / (uint32_t)W), x = (int)(p - (uint32_t)y * (uint32_t)W);
    const size_t fo = (size_t)blockIdx.y * NP;
    const int x2 = clampi(x + dir * (d_min + (int)d), 0, W - 1);             // :368-375 with Pd0 = (x + 1 + dir * d_min, y + 1), u = (dir, 0)
    Craw[fo * D + gid] = (uint8_t)__popc(cen1[fo + p] ^ cen2[fo + (size_t)y * W + x2]);   // :377-378
}

// Window words of the fused kernel (see its comment): with xq = xs - 2 + lane the lane's raw column and px = clamp(xq, 0, W - 1),
// word (px - xb) + dir * d lies in [0, REACH) for every d < D.  Above: px <= xq, so the word is at most lane + D - 1 <= REACH - 1.
// Below: px >= min(xq, xs) -- the clamp at W - 1 never goes below xs, a strip starts inside the image, and the clamp at 0 only
// raises px -- and xq >= xs - 2 = xb (dir +1) or xb + D - 1 (dir -1), so the word is >= 0 (the two left apron lanes of a strip
// reach words 0 and 1).  Copy c of the window holds every word from c upwards at index word - c, and a lane reads copy s & 3
// from s - (s & 3) >= 0 on, 16 words up to s + 15 <= REACH - 1: all written.  The window itself is filled with the clamp on the
// image columns, so a word's content is cen2[y][clamp(px + dir * d)].
//
// A search range that starts at d_min (index d = disparity d_min + d): the sample is cen2[y][clamp(px + dir * (d_min + d))], the
// sample of the unshifted range dir * d_min columns further on.  The kernel keeps xb, the word index (px - xb) + dir * d and so
// every bound above -- none of them mentions what a word holds -- and fills word i with cen2[y][clamp(xb + dir * d_min + i)]
// instead of cen2[y][clamp(xb + i)]: the word the lane reads then holds cen2[y][clamp(xb + dir * d_min + (px - xb) + dir * d)] =
// cen2[y][clamp(px + dir * (d_min + d))].  That is why the four-copy layout, PITCH, the copies' alignment and the [0, REACH)
// word bounds are untouched: they are properties of word INDICES, which depend on lane, strip, dir and d alone.  What does
// change is the fill's address, xb + dir * d_min + i with i < REACH: it can now leave the image on EITHER side (dir = -1 with a
// negative d_min runs off the right edge, as dir = +1 always could; |d_min| > W + REACH puts every word at one clamped column),
// so the fill clamps to [0, W - 1] on both sides -- one clampi, as before -- and reads row[0 .. W - 1] only.  |dir * d_min| <=
// 1024 (the entry points refuse more) and |xb + i| < 2^22 + 2^9, so the sum cannot wrap.
void launch_stereo_cost(hipStream_t st, const uint32_t* cen1, const uint32_t* cen2, uint8_t* Craw, uint8_t* C, int W, int H, int D,
                        int direction, int frames, int d_min) {
    const int dir = direction < 0 ? -1 : 1;
    const CostKernels k = select_cost_kernels(W, H, D, true);                // (FSGM_COST_FUSED=0: the two-kernel form, as for launch_epi_cost)
    if (k.raw == COST_RAW_FUSED) {
        EpiCostArgs a{};
        a.cen1 = cen1; a.cen2 = cen2; a.W = W; a.H = H; a.D = D;
        launch_costbox(st, a, C, frames, dir, dir * d_min);
        return;
    }
    const size_t n = (size_t)W * H * D;                                      // < 2^31 (plan creation)
    hipLaunchKernelGGL(stereo_rawcost_kernel, dim3((unsigned)((n + 255) / 256), frames), dim3(256), 0, st, cen1, cen2, Craw, W, H, D, dir, d_min);
    launch_box5x5(st, k.box, Craw, C, W, H, D, frames);
}

// The outputs of a search range that starts at d_min as true disparities: candidate index * 256 (+ the parabola's offset) becomes
// the int32 256 * d_min + value, and the second view's invalid marker 512 << 8 -- a valid value once d_min > 0 -- INT32_MIN.
// In place, one thread per pixel of the whole batch; disp2 null without the forward-backward check.
__global__ __launch_bounds__(256) void stereo_range_kernel(uint32_t* __restrict__ disp, uint32_t* __restrict__ disp2, size_t n, int base) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    disp[i] = (uint32_t)(base + (int)disp[i]);
    if (disp2) {
        const uint32_t v = disp2[i];
        disp2[i] = v == (512u << 8) ? 0x80000000u : (uint32_t)(base + (int)v);
    }
}

void launch_stereo_range(hipStream_t st, uint32_t* disp, uint32_t* disp2, size_t n, int d_min) {
    hipLaunchKernelGGL(stereo_range_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, disp, disp2, n, 256 * d_min);
}

}  // namespace fsgm
