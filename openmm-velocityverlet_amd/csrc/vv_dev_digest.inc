// vv_dev_digest.inc -- part of vv_device.inc: the state digest (vvhip_state_digest; include/vvhip.h states the definition).  One
// stand-alone streaming reduction per section that reads the section's words and adds to its own scratch word (DigestArgs::out), and
// nothing else: no accumulator, no thermostat copy, no status word.
//   every thread strides over the section's 16-byte groups (from the first 16-byte boundary on) and keeps one uint64 partial; the ragged
//   ends -- up to three words in front of that boundary, up to three behind the last whole group -- are single-word loads of the grid's
//   first threads; wave reduction, the block's waves through LDS, one 64-bit integer atomic per block.
// Wrapping integer adds: the same bits for any grid, block size or order of arrival.

__device__ __forceinline__ unsigned long long dg_mix(unsigned long long g, unsigned int w) {
    unsigned long long z = ((g << 32) | (unsigned long long) w) + 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(512) vv_kernel_digest(const DigestArgs a) {
    __shared__ unsigned long long part[8];
    const unsigned long long n = a.nwords;
    const unsigned long long to_boundary = ((16u - (unsigned) ((unsigned long long) a.words & 15u)) & 15u) >> 2;
    const unsigned long long head = to_boundary < n ? to_boundary : n;
    const unsigned long long nvec = (n - head) >> 2, tail0 = head + 4 * nvec;
    const uint4* v = (const uint4*) (a.words + head);
    const unsigned long long tid = (unsigned long long) blockIdx.x * blockDim.x + threadIdx.x, stride = (unsigned long long) gridDim.x * blockDim.x;
    unsigned long long s = 0;
    for (unsigned long long i = tid; i < nvec; i += stride) {
        const uint4 q = v[i];
        const unsigned long long g = a.base + head + 4 * i;
        s += dg_mix(g, q.x) + dg_mix(g + 1, q.y) + dg_mix(g + 2, q.z) + dg_mix(g + 3, q.w);
    }
    if (tid < head) s += dg_mix(a.base + tid, a.words[tid]);
    if (tid < n - tail0) s += dg_mix(a.base + tail0 + tid, a.words[tail0 + tid]);
    const long long t = rep_wave_sum((long long) s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = (unsigned long long) t;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = 0;
        for (int w = 0; w < (int) (blockDim.x >> 6); w++) b += part[w];
        if (b) atomicAdd(a.out, b);
    }
}
#endif
