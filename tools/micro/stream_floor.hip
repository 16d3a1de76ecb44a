// Microbenchmark: the load-only floor of the striped 8-byte scan (scan_values_kernel<2,1,F>).
// Same grid (768 x 256), same 2048-row tile interleave (workgroup g reads tiles g, g + G, ...), same loads per
// tile and lane (four `nt` buffer_load_dwordx4 of the values, the next tile's issued ahead of the current tile's
// use; the validity words on the default cache policy), over one column of 1e9 rows (8 GB of values + 125 MB of
// bitmap). The fold is replaced by an OR into one register pair per lane, stored once at the end so the loads
// survive. VALIDITY=1 reads the bitmap as four dwordx2 loads per lane (the scan's gather), VALIDITY=2 as four byte
// loads (tried in r08), VALIDITY=0 not at all. Reports ms per column and TB/s for each, then the dwordx2 variant
// again at 1024 and 1536 workgroups (4 and 6 waves per SIMD in flight instead of 3): what more loads in flight buy.
// WORK = 96 ... 384 adds that many v_fma_f64 per tile and lane on the loaded values (8 independent chains) at the
// scan's grid: what a fold of that many VALU instructions costs on top of the loads at 3 waves per SIMD. PIPE
// requests the validity words ahead of the next tile's values, so the next tile stays in flight during the work.
// Results and their reading: profiles/r08/c2_stream_floor.txt.
//   hipcc -O3 --offload-arch=gfx950 stream_floor.hip -o stream_floor && ./stream_floor
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

constexpr int kBlock = 256;
constexpr int kTileRows = 2048;
constexpr int kGrid = 768;

typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v2i_t __attribute__((ext_vector_type(2)));

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void* base, int64_t byte_off, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)base + byte_off), (short)0, bytes, 0x00020000);
}

__device__ __forceinline__ void load_tile(const uint64_t* values, int64_t tile, int tid, v4i_t (&x)[4]) {
    const __amdgpu_buffer_rsrc_t r = tile_rsrc(values, tile * kTileRows * 8, kTileRows * 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = __builtin_amdgcn_raw_buffer_load_b128(r, tid * 16, i * 4096, 2 /* nt */);
}

// Every descriptor covers exactly one full tile, and the loop below visits full tiles only (t < nfull), so no lane
// reads outside [values, values + nfull * 16 KiB) or [bitmap, bitmap + nfull * 256 B).
template <int VALIDITY, int WORK = 0, bool PIPE = false>
__global__ void __launch_bounds__(kBlock) stream_kernel(const uint64_t* __restrict__ values,
                                                        const uint64_t* __restrict__ bitmap, int64_t nfull,
                                                        uint64_t* __restrict__ out) {
    const int tid = threadIdx.x;
    const int64_t G = gridDim.x;
    uint32_t lo = 0, hi = 0;
    v4i_t x[4], xn[4];
    int64_t t = blockIdx.x;
    if (t < nfull) load_tile(values, t, tid, x);
    for (; t < nfull; t += G) {
        const int64_t tn = t + G;
        if (PIPE) {
            // The current tile's validity words are requested before the next tile's values: loads retire in order,
            // so the wait for the words (vmcnt(4)) leaves the next tile in flight while this one is worked on.
            const __amdgpu_buffer_rsrc_t r = tile_rsrc(bitmap, t * (kTileRows / 8), kTileRows / 8);
            v2i_t w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rel = j * (kBlock * 2) + tid * 2;
                w[j] = __builtin_amdgcn_raw_buffer_load_b64(r, (rel >> 6) * 8, 0, 0);
            }
            // no branch around the value loads (the last iteration reads its own tile again): a conditional block
            // is placed ahead of the validity loads by the compiler, which puts the order back to what it was
            __builtin_amdgcn_sched_barrier(0);
            load_tile(values, tn < nfull ? tn : t, tid, xn);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo |= (uint32_t)w[j].x;
                hi |= (uint32_t)w[j].y;
            }
        } else if (tn < nfull) {
            load_tile(values, tn, tid, xn);
        }
        if (VALIDITY && !PIPE) {
            const __amdgpu_buffer_rsrc_t r = tile_rsrc(bitmap, t * (kTileRows / 8), kTileRows / 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (VALIDITY == 1) {
                    const int rel = j * (kBlock * 2) + tid * 2;
                    const v2i_t w = __builtin_amdgcn_raw_buffer_load_b64(r, (rel >> 6) * 8, 0, 0);
                    lo |= (uint32_t)w.x;
                    hi |= (uint32_t)w.y;
                } else {
                    lo |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(r, tid >> 2, j * 64, 0);
                }
            }
        }
        if (WORK) {
            double a[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[2 * i] = __builtin_bit_cast(double, ((uint64_t)(uint32_t)x[i].y << 32) | (uint32_t)x[i].x);
                a[2 * i + 1] = __builtin_bit_cast(double, ((uint64_t)(uint32_t)x[i].w << 32) | (uint32_t)x[i].z);
            }
            const double c = __builtin_bit_cast(double, (uint64_t)tid);
#pragma unroll
            for (int r = 0; r < WORK / 8; ++r)
#pragma unroll
                for (int i = 0; i < 8; ++i) asm volatile("v_fma_f64 %0, %0, %0, %1" : "+v"(a[i]) : "v"(c));
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                lo |= (uint32_t)__builtin_bit_cast(uint64_t, a[i]);
                hi |= (uint32_t)(__builtin_bit_cast(uint64_t, a[i]) >> 32);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lo |= (uint32_t)(x[i].x | x[i].z);
            hi |= (uint32_t)(x[i].y | x[i].w);
            x[i] = xn[i];
        }
    }
    out[(int64_t)blockIdx.x * kBlock + tid] = ((uint64_t)hi << 32) | lo;
}

__global__ void fill_kernel(uint64_t* p, int64_t n, uint64_t seed) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = (uint64_t)i * 0x9E3779B97F4A7C15ull + seed;
}

int main() {
    const int64_t rows = 1000000000;
    const int64_t nfull = rows / kTileRows;
    const int64_t vwords = nfull * kTileRows, bwords = nfull * (kTileRows / 64);
    uint64_t *values, *bitmap, *out;
    CHECK(hipMalloc(&values, vwords * 8));
    CHECK(hipMalloc(&bitmap, bwords * 8));
    const int grids[] = {kGrid, 1024, 1536};
    CHECK(hipMalloc(&out, (size_t)1536 * kBlock * 8));
    fill_kernel<<<4096, 256>>>(values, vwords, 1);
    fill_kernel<<<4096, 256>>>(bitmap, bwords, 2);
    CHECK(hipDeviceSynchronize());
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    typedef void (*kfn)(const uint64_t*, const uint64_t*, int64_t, uint64_t*);
    struct { const char* name; kfn f; double bytes; int grid; } ks[] = {
        {"values only", stream_kernel<0>, (double)vwords * 8, grids[0]},
        {"values + validity (4 x dwordx2 per lane)", stream_kernel<1>, (double)(vwords + bwords) * 8, grids[0]},
        {"values + validity (4 x byte per lane)", stream_kernel<2>, (double)(vwords + bwords) * 8, grids[0]},
        {"values + validity (dwordx2), grid 1024", stream_kernel<1>, (double)(vwords + bwords) * 8, grids[1]},
        {"values + validity (dwordx2), grid 1536", stream_kernel<1>, (double)(vwords + bwords) * 8, grids[2]},
        {"dwordx2 validity + 96 v_fma_f64 per tile", stream_kernel<1, 96>, (double)(vwords + bwords) * 8, grids[0]},
        {"dwordx2 validity + 192 v_fma_f64 per tile", stream_kernel<1, 192>, (double)(vwords + bwords) * 8, grids[0]},
        {"dwordx2 validity + 288 v_fma_f64 per tile", stream_kernel<1, 288>, (double)(vwords + bwords) * 8, grids[0]},
        {"dwordx2 validity + 384 v_fma_f64 per tile", stream_kernel<1, 384>, (double)(vwords + bwords) * 8, grids[0]},
        {"validity first, 0 v_fma_f64", stream_kernel<1, 0, true>, (double)(vwords + bwords) * 8, grids[0]},
        {"validity first, 192 v_fma_f64", stream_kernel<1, 192, true>, (double)(vwords + bwords) * 8, grids[0]},
        {"validity first, 288 v_fma_f64", stream_kernel<1, 288, true>, (double)(vwords + bwords) * 8, grids[0]}};
    const int reps = 21;
    printf("grid %d x %d, %lld full tiles of %d rows, %d timed launches per variant after 3 untimed\n", kGrid, kBlock,
           (long long)nfull, kTileRows, reps);
    for (auto& k : ks) {
        std::vector<float> ms;
        for (int r = 0; r < reps + 3; ++r) {
            CHECK(hipEventRecord(a));
            hipLaunchKernelGGL(k.f, dim3(k.grid), dim3(kBlock), 0, 0, values, bitmap, nfull, out);
            CHECK(hipEventRecord(b));
            CHECK(hipEventSynchronize(b));
            float t;
            CHECK(hipEventElapsedTime(&t, a, b));
            if (r >= 3) ms.push_back(t);
        }
        CHECK(hipGetLastError());
        std::sort(ms.begin(), ms.end());
        const float mn = ms.front(), md = ms[ms.size() / 2], mx = ms.back();
        printf("%-42s %.3f GB  min %.4f  median %.4f  max %.4f ms  -> %.3f TB/s at the median (%.3f at the min)\n",
               k.name, k.bytes * 1e-9, mn, md, mx, k.bytes / (md * 1e-3) * 1e-12, k.bytes / (mn * 1e-3) * 1e-12);
    }
    return 0;
}
