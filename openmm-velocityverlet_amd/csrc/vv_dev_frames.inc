// vv_dev_frames.inc -- part of vv_device.inc: trajectory frames (vvhip_frames_*; include/vvhip.h states layout, values and schedule).
// Two stand-alone kernels that read posq, posqCorrection and velm and write the recorder's own buffer and cursor, and nothing else: no
// force, no accumulator, no thermostat copy, no rendezvous or status word.
//   frame:    one thread per recorded particle, striding over a capped grid.  Per particle one 16- or 32-byte load of posq (and of the
//             correction in mixed precision), one of velm if velocities are recorded, a 4-byte index load only with a subset (without
//             one the index is the thread's own), and one store per component plane: lane i of a wave stores element i of the plane, a
//             contiguous 4- or 8-byte-per-lane stream, no LDS staging.  Every thread reads the frame index from the device-side cursor;
//             nothing writes that word while this kernel runs.  With the cursor at or past the capacity nothing is stored.
//   advance:  one thread behind it (the kernel boundary orders it behind every block's read of the cursor): writes the frame's header
//             if the frame was stored, counts it as dropped if not, and advances the cursor either way -- no memset node, no host work.
// The tails need no special case: the loop bound is the particle count, the padding elements of a plane are never written (zero since the
// buffer was allocated), and a shard without recorded particles runs one idle block and the advance.

template <class real, class mixed, class out_t, bool SUBSET>
__global__ void __launch_bounds__(512) vv_kernel_frame(const FrameArgs a) {
    using real4 = typename Vec<real>::v4;
    using mixed4 = typename Vec<mixed>::v4;
    constexpr bool CORR = sizeof(real) != sizeof(mixed);      // mixed precision: the position is posq + posqCorrection, summed in double
    const unsigned long long c = __hip_atomic_load(&a.cursor[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c >= (unsigned long long) a.capacity) return;
    unsigned char* frame = a.frames + (size_t) c * (size_t) a.frame_bytes;
    out_t* px = a.off_positions >= 0 ? (out_t*) (frame + a.off_positions) : nullptr;
    out_t* vx = a.off_velocities >= 0 ? (out_t*) (frame + a.off_velocities) : nullptr;
    const size_t ps = (size_t) a.plane_stride;
    const long long stride = (long long) gridDim.x * blockDim.x;
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        const int k = SUBSET ? a.subset[i] : i;
        if (px) {
            const real4 p = ((const real4*) a.posq)[k];
            if (CORR) {
                const real4 q = ((const real4*) a.corr)[k];
                px[i] = (out_t) ((double) p.x + (double) q.x);
                px[ps + i] = (out_t) ((double) p.y + (double) q.y);
                px[2 * ps + i] = (out_t) ((double) p.z + (double) q.z);
            } else {
                px[i] = (out_t) p.x; px[ps + i] = (out_t) p.y; px[2 * ps + i] = (out_t) p.z;
            }
        }
        if (vx) {
            const mixed4 v = ((const mixed4*) a.velm)[k];
            vx[i] = (out_t) v.x; vx[ps + i] = (out_t) v.y; vx[2 * ps + i] = (out_t) v.z;
        }
    }
}

#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(64) vv_kernel_frame_advance(const FrameArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long c = a.cursor[0];
    if (c < (unsigned long long) a.capacity) {
        vvhip_frame_header* h = (vvhip_frame_header*) (a.frames + (size_t) c * (size_t) a.frame_bytes);
        h->ordinal = (int64_t) c; h->reserved = 0;
        for (int k = 0; k < 3; k++) { h->box[k] = a.box[k]; h->pad[k] = 0.0; }
    } else {
        a.cursor[1] = a.cursor[1] + 1;
    }
    a.cursor[0] = c + 1;
}
#endif
