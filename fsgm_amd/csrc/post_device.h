// post_device.h -- device helpers shared by the scalar post-processing kernels (post_kernels.hip) and the two-channel flow
// chain (flow_post_kernels.hip): the lock-free union-find of the connected-component labelling and the row scan of the
// hole fill.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsgm {

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
