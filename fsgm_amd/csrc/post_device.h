// post_device.h -- device helpers of the post-processing kernels (post_kernels.hip), which run on scalar maps (CH = 1) and
// on two-channel flows (CH = 2) alike: where a pixel's channels live and the two rules that depend on the channel count
// ("valid", "joins"), the lock-free union-find of the connected-component labelling and the row scan of the hole fill.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsgm {

#define FSGM_NAN __longlong_as_double(0x7FF8000000000000LL)

// A batch of CH-channel maps is f64 [nf][CH][H][W].  Pixel g = f*NP + p of the union-find (frame f, NP = W*H) has its
// first channel at f*CH*NP + p and channel c c*NP further: for a scalar map that is g itself (no frame needed, i32 as g).
template <int CH, class I>
__device__ __forceinline__ auto px_first(I g, I f, size_t NP) {
    if constexpr (CH == 1) return g;
    else return (size_t)g + (size_t)f * (CH - 1) * NP;
}
template <int CH>
__device__ __forceinline__ auto px_first(int g, int NP) {
    if constexpr (CH == 1) return g;
    else return px_first<CH>(g, g / NP, (size_t)NP);
}

template <int CH>
struct Px { double c[CH]; };
template <int CH>
__device__ __forceinline__ Px<CH> px_load(const double* first, size_t NP) {
    Px<CH> v;
#pragma unroll
    for (int c = 0; c < CH; c++) v.c[c] = first[c * NP];
    return v;
}
// valid: no channel is NaN (of a loaded pixel; of the pixel whose first channel is at `first`, a later channel read only
// behind a number)
template <int CH>
__device__ __forceinline__ bool px_valid(const double* first, size_t NP) {
#pragma unroll
    for (int c = 0; c < CH; c++)
        if (isnan(first[c * NP])) return false;
    return true;
}
template <int CH>
__device__ __forceinline__ bool px_valid(const Px<CH>& v) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < CH; c++) ok = ok && !isnan(v.c[c]);
    return ok;
}
// speckle_filter.m:55 for a valid pixel a and its neighbour b: b valid and |a - b| < maxDiff, in every channel, all strict
template <int CH>
__device__ __forceinline__ bool px_joins(const Px<CH>& a, const Px<CH>& b, double maxDiff) {
    bool j = px_valid(b);
#pragma unroll
    for (int c = 0; c < CH; c++) j = j && fabs(__dsub_rn(a.c[c], b.c[c])) < maxDiff;
    return j;
}

__device__ __forceinline__ int ccl_find(int32_t* parent, int i) {
    int p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != i) {
        i = p;
        p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return i;
}

__device__ __forceinline__ void ccl_union(int32_t* parent, int a, int b) {
    while (true) {
        a = ccl_find(parent, a);
        b = ccl_find(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }            // hang the larger root under the smaller
        const int old = atomicMin(&parent[b], a);
        if (old == b) return;                                    // b was still a root: joined
        b = old;                                                 // somebody re-parented b meanwhile: retry from there
    }
}

// speckle_filter.m:48 regionPixelNum: size[root] += 1 for every valid lane.  Neighbouring pixels mostly share a root, and one
// big region would otherwise serialise hundreds of thousands of atomics on a single counter: add once per distinct root per
// wave.  Every lane of the wave must call it (r is the lane's root, read only where valid).
__device__ __forceinline__ void ccl_add_sizes(bool valid, int r, int32_t* size) {
    unsigned long long todo = __builtin_amdgcn_ballot_w64(valid);
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const int lr = __builtin_amdgcn_readlane(r, leader);
        const unsigned long long same = __builtin_amdgcn_ballot_w64(valid && r == lr) & todo;
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&size[lr], __popcll(same));
        todo &= ~same;
    }
}

__device__ __forceinline__ int block_scan_max_256(int v, int* sh) {      // inclusive, in thread order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int t = __shfl_up(v, s);
        if (lane >= s) v = max(v, t);
    }
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    int pre = INT32_MIN;
    for (int w = 0; w < wave; w++) pre = max(pre, sh[w]);
    __syncthreads();
    return max(v, pre);
}

}  // namespace fsgm
