// ng_kernels.h -- launch interface of the neighbour-guided variants
// (calc_pyd_cost_sgm_ng.cpp and calc_cost_sgm_ng.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <array>

#define FSGM_NG_MAX_D 512        // candidates per pixel of the hint-map variant: 9*(2r+1)^2, r <= 3

namespace fsgm {

struct Cand { int32_t mvx, mvy, cost; };     // calc_pyd_cost_sgm_ng.cpp:32-37

struct NgCostArgs {
    const uint32_t* cen1;   // [frames][NP]
    const uint32_t* cen2;
    const double* mv;       // [frames][2][mvH*mvW]
    Cand* C;                // [frames][NP][D]
    uint32_t* K4;           // [frames][NP][D] 4-byte entries (ng_key4) -- the 3x3 hint kernel's output when every key fits; null: 12-byte entries only
    uint32_t* flags;        // two words zeroed by the caller, = { unsafe, a key that does not fit 4 bytes }; needed with K4
    uint32_t* unsafe;       // one word (may be null), zeroed by the caller: set when a motion vector has |v| >= 2^30
    int W, H, mvW, mvH;
    int rAgg, rX, rY;
};

struct NgAggArgs {
    const Cand* C;          // [frames][NP][D]
    uint32_t* S;            // [frames][NP][D], zeroed before the launch; paths add atomically
    const uint32_t* unsafe; // the cost kernel's flag (null: take the generic kernel)
    const uint16_t* dd;     // [frames][NP][D] place of a candidate in its pixel's list without repeats, 0xFFFF = a repeat
    const uint8_t* dk;      //                 (launch_ng_dedupe); [frames][NP] length of that list.  Null: every candidate is staged
    const uint32_t* dbox;   // [frames][NP] packed origin of the bounding box of a pixel's motion vectors, or all ones when it is larger
                            // than the grid matcher takes (launch_ng_dedupe); null: list matcher only
    const uint32_t* ck;     // [frames][NP][D] packed motion vector (ng_pack_mv) of the kept entry at each place   } launch_ng_dedupe; the
    const uint16_t* cm;     // [frames][NP][D] (index of the group's first member << 8) | cost of the kept entry     } compact kernel's input
    int me;                 // this kernel's matcher id (NG_COMPACT16 ...): it runs when kstat's choice word names it; NG_ANY: it always runs
    int blk_begin_c[5];     // compact kernel: first block of each range (4 lines a workgroup)
    int slot_of_c[4];
    int16_t* L4;            // [frames][NP][4 path slots][64] the compact kernel's path costs of the kept entries, by place in the pixel's list:
                            // plain 2-byte stores, contiguous per pixel and path, instead of one atomic add to S per kept entry and path
                            // (208 M scattered atomics per batch of 8 at 1242x375: 1.6 of 8.3 ms).  The WTA sums the four slots.
                            // Null: the compact kernel is not launched
    uint32_t* kstat;        // [0, 256) partial sums of the list lengths of a sample of this launch's pixels; [NG_KSTAT_FLAGS] bit 0 a list longer
                            // than 64 entries, bit 1 a pixel whose entries do not fit the packed key (launch_ng_dedupe); [NG_KSTAT_CHOICE] the
                            // id of the matcher that runs (ng_decide_kernel; a compact id: S holds nothing, the sums are in L4)
    int W, H, D;
    int P1, P2;
    int blk_begin[5];
    int slot_of[4];         // split kernel: path slot of block range k (long lines are launched first)
};

struct NgWtaArgs {
    const Cand* C;
    const uint32_t* S;
    const uint16_t* cm;     // launch_ng_dedupe's kept-entry table and list lengths: the search runs over the groups of repeats,
    const uint8_t* dk;      // whose sums sit at their first members' indices; both null: over all D candidates
    const int16_t* L4;      // the compact kernel's per-path costs and the launch's statistics words (the choice word a compact id: sums =
    const uint32_t* kstat;  // the four slots of L4 at the entry's place; else S); null: S
    const uint32_t* K4;     // 4-byte entries and the cost kernel's flags (flags[1] == 0: every key fits): the winner's motion vector comes
    const uint32_t* flags;  // from its key when the compact kernel ran; null: from C
    uint32_t* minC;         // [frames][NP]
    double* flow;           // [frames][2][NP]
    int W, H, D;
    uint32_t* minC2 = nullptr;   // optional runner-up cost [frames][NP] (FSGM_NO_RUNNER_UP of include/fsgm.h, the neighbour-guided rule);
                                 // null: the kernel without it
};

struct NgSubpixArgs {
    const uint32_t* cen1;
    const uint32_t* cen2;
    double* flow;
    int W, H;
};

// on-the-fly variant (calc_cost_sgm_ng.cpp): one workgroup walks one frame in raster order
constexpr int OTF_D = 108;       // DIRECTION_NUM*(N+M)*MV_PER_HINT  (:194)
constexpr int OTF_E = 110;       // + N best entries                  (:196)
struct OtfArgs {
    const uint8_t* I1;      // [frames][NP]
    const uint32_t* cen1;
    const uint32_t* cen2;
    const int32_t* rnd;     // [frames][NP*8]  libc rand() stream, 2 draws per random hint
    Cand* Lrow;             // [frames][3][2][W][OTF_E]  L2, L3, L4 double row buffers (zeroed)
    uint32_t* minC;         // [frames][NP]
    double* flow;           // [frames][2][NP]
    int W, H, P1, P2;
    int exact;              // 1: start in the exact matcher (FSGM_OTF_EXACT=1; otherwise entered when a motion vector leaves the packed range)
};

// The aggregation kernels of a level with D <= 128.  NG_ANY: the level's only matcher; NG_REST: the split or
// lines kernel next to the compact kernels, when the grid kernel is not in the set; NG_LIST: the lines kernel next to the grid kernel
enum { NG_ANY = 0, NG_COMPACT16 = 1, NG_COMPACT32 = 2, NG_COMPACT64 = 3, NG_GRID = 4, NG_LIST = 5, NG_REST = 6 };
__host__ __device__ inline bool ng_is_compact(uint32_t id) { return id >= NG_COMPACT16 && id <= NG_COMPACT64; }
constexpr int NG_KSTAT_FLAGS = 256, NG_KSTAT_CHOICE = 257, NG_KSTAT_WORDS = 258;
constexpr int NG_L4_PER_PIXEL = 4 * 64;      // int16 entries of L4 per pixel

// Scratch of one level of the hint-map variant for all frames of a batch (frame-major); ng_level_bufs sizes it
struct NgLevelBufs {
    uint32_t *cen1, *cen2;  // census of both images
    Cand* C;                // candidate lists
    uint32_t* S;            // sums; the 4-byte entries until the matchers need S
    uint32_t* unsafe;       // the cost kernel's two flag words
    uint16_t* dd;           // launch_ng_dedupe's tables (NgAggArgs): dd, dk, dbox, kstat, ck, cm
    uint8_t* dk;
    uint32_t* box;
    uint32_t* kstat;
    uint32_t* ck;
    uint16_t* cm;
    int16_t* L4;            // the compact kernel's per-path costs (D <= 128; 0 bytes otherwise)
};
struct NgBuf { void** slot; size_t bytes; };
// every slot of `b` with its size in bytes for `frames` frames of W x H pixels and D candidates: the caller carves or allocates them
std::array<NgBuf, 12> ng_level_bufs(NgLevelBufs& b, int W, int H, int D, int frames);

// One level of calc_pyd_cost_sgm_ng (:470-517) for all frames of a batch: caller-owned images, hint map and results
struct NgLevel {
    const uint8_t* I1;      // [frames][H][W]
    const uint8_t* I2;
    const double* mv;       // [frames][2][mvH][mvW]
    uint32_t* minC;         // [frames][H][W]
    double* flow;           // [frames][2][H][W]
    int W, H, mvW, mvH;
    int r, rAgg;            // halfSearchWinSize, aggSize / 2: D = 9 (2r+1)^2 candidates
    int P1, P2;
    int subPixelRefine;
    uint32_t* minC2 = nullptr;   // [frames][H][W] the WTA's runner-up cost, when asked for (NgWtaArgs)
};
// The aggregation kernels a level launches: ng_matcher_set fills it from the level's shape, its frame count and the
// A/B switches, once per level enqueue.  With more than one member the device picks: ng_decide_kernel feeds the dedupe kernel's
// statistics to ng_choose and leaves the id in kstat's choice word, and every matcher returns unless the word names it.
struct NgMatcherSet {
    bool plain;             // D > 128: ng_agg_kernel, the only member
    bool compact;           // the compact kernels.  They walk a frame with 32-bit byte offsets (entries x 4 bytes, pixels x 512 bytes
                            // of L4): not for W*H*D >= 2^30 or W*H >= 2^23
    int compact_g;          // 16 / 32 / 64: that lanes-a-line class is the only compact member (FSGM_NG_COMPACT_G); 0: all three
    bool grid, grid_only;   // the grid kernel is a member / the only one (FSGM_NG_GRID=1)
    int parts;              // the split kernel's parts (2 .. 4: FSGM_NG_SPLIT, one or two frames); 1: the lines kernel
    bool device_choice() const { return compact || (grid && !grid_only); }
};
// the dedupe kernel's sample of n pixels: every 16th workgroup of 4 pixels
__host__ __device__ inline unsigned long long ng_sample_pixels(unsigned long long n) { return (((n + 3) / 4 + 15) / 16) * 4; }
// The rule: which member runs, from the sum of the sampled list lengths, the sample's pixel count and kstat's flags word.
// Compact (one wave per 64/G lines over the kept entries only, work ~ K^2): every list <= 64 entries and inside the packed key's
// range, mean length below 40; its class by the mean length for batches (throughput: more lines a wave), 64 lanes for one or two
// frames (their long lines are serial chains: one line a wave is the shortest step); a forced class still steps aside for lists
// it cannot hold.  Otherwise grid from a mean length of 16 (it costs the same at any length), list below it.
constexpr int NG_GRID_MIN_K = 16;   // (also ng_matcher_set: with fewer candidates than this the grid kernel is no member)
__host__ __device__ inline uint32_t ng_choose(const NgMatcherSet& ms, int frames, unsigned long long sum, unsigned long long npix, uint32_t flags) {
    constexpr unsigned long long NG_COMPACT_MAX_K = 40;
    if (ms.compact && (flags & 3u) == 0u && sum < NG_COMPACT_MAX_K * npix) {
        if (ms.compact_g) return ms.compact_g == 16 ? NG_COMPACT16 : ms.compact_g == 32 ? NG_COMPACT32 : NG_COMPACT64;
        return frames <= 2 ? NG_COMPACT64 : sum < 14 * npix ? NG_COMPACT16 : sum < 28 * npix ? NG_COMPACT32 : NG_COMPACT64;
    }
    if (ms.grid_only) return NG_GRID;
    if (ms.grid) return sum >= (unsigned long long)NG_GRID_MIN_K * npix ? NG_GRID : NG_LIST;
    return ms.compact ? NG_REST : NG_ANY;
}
// "compact16" / "compact32" / "compact64", "grid", "list", "split2" .. "split4", "lines", "generic": the kernel behind an id of this set
const char* ng_matcher_name(const NgMatcherSet& ms, uint32_t id);
// what the rule answers for a level of this shape under the current FSGM_NG_* environment: no device needed
const char* ng_auto_matcher(int W, int H, int D, int frames, unsigned long long sum, unsigned long long npix, uint32_t flags);

// the largest dynamic LDS request, in bytes, among the kernels such a level launches under the current environment (no device
// needed); ng_level_enqueue returns hipErrorInvalidConfiguration, with nothing queued, for a level whose request exceeds 64 KiB
size_t ng_auto_matcher_lds(int W, int H, int D, int frames);

// Queues the level on `st`: census of both images, candidate costs, repeat removal, matcher, WTA and, when asked, the census
// sub-pixel step.  Reads the A/B switches and decides the 4-byte entries.  With D <= 128 the matchers leave
// S incomplete: a caller that reads S back queues launch_ng_l4_to_s and launch_ng_fill_repeats behind the level.
// `used` (may be null): the level's matcher set, for fsgm_ng_last_decision.
hipError_t ng_level_enqueue(hipStream_t st, const NgLevelBufs& b, const NgLevel& lv, int frames, NgMatcherSet* used = nullptr);
// S of the repeats := S of the entries they repeat (only needed when S itself is read back: the WTA looks them up)
void launch_ng_fill_repeats(hipStream_t st, uint32_t* S, const uint16_t* dd, const uint16_t* cm, int W, int H, int D, int frames);
// S at the kept entries' first-member indices := the sum of L4's four slots, when a compact kernel ran (kstat's choice word): only for reading S back
void launch_ng_l4_to_s(hipStream_t st, uint32_t* S, const int16_t* L4, const uint16_t* cm, const uint8_t* dk, const uint32_t* kstat, int W, int H, int D, int frames);
void launch_otf(hipStream_t st, const OtfArgs& a, int frames);

}  // namespace fsgm
