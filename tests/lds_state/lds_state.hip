// TEST INFRASTRUCTURE ONLY (tests/lds_state.py): put the LDS of every CU into a
// known state before a kernel under test, read that state back, and one toy
// kernel that is wrong on purpose.  Each entry point only launches: no wait
// loop, no grid barrier, no spin.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LDS_BYTES 163840  // the whole LDS of a CU: one resident block per CU
#define LDS_WORDS (LDS_BYTES / 4)
#define LDS_THREADS 256

// s_getreg_b32 immediates: id | offset << 6 | (size - 1) << 11
#define GETREG_HW_ID ((31 << 11) | 4)        // HW_REG_HW_ID, all 32 bits
#define GETREG_XCC_ID ((3 << 11) | 20)       // HW_REG_XCC_ID, bits 3:0

__global__ __launch_bounds__(LDS_THREADS) void lds_fill_kernel(uint32_t pattern) {
    extern __shared__ __attribute__((aligned(16))) uint32_t w[];
    uint4 v = make_uint4(pattern, pattern, pattern, pattern);
    for (int i = threadIdx.x; i < LDS_WORDS / 4; i += LDS_THREADS) reinterpret_cast<uint4 *>(w)[i] = v;
    // the stores above have no reader in this kernel: keep them
    __asm__ volatile("" ::: "memory");
}

// HW_REG_HW_ID (gfx9 family): CU_ID 11:8, SH_ID 12, SE_ID 15:13.  The key is
// XCC_ID << 8 | those eight bits: one value per CU of the device.
__global__ __launch_bounds__(LDS_THREADS) void lds_probe_kernel(uint32_t pattern, uint32_t *key_out,
                                                                uint32_t *bad_out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t w[];
    uint32_t bad = 0;
    for (int i = threadIdx.x; i < LDS_WORDS / 4; i += LDS_THREADS) {
        const uint4 v = reinterpret_cast<const uint4 *>(w)[i];
        bad += (v.x != pattern) + (v.y != pattern) + (v.z != pattern) + (v.w != pattern);
    }
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o, 64);
    // nothing is written to LDS: the four waves add their counts in global memory (bad_out starts at 0)
    if ((threadIdx.x & 63) == 0) atomicAdd(&bad_out[blockIdx.x], bad);
    if (threadIdx.x == 0) {
        const uint32_t hw = __builtin_amdgcn_s_getreg(GETREG_HW_ID);
        const uint32_t xcc = __builtin_amdgcn_s_getreg(GETREG_XCC_ID);
        key_out[blockIdx.x] = (xcc << 8) | ((hw >> 8) & 0xffu);
    }
}

// Wrong on purpose: t[PLANT_N - 1] is never staged, and 0.0f * (that word) is
// added to an exact sum.  0 x finite = 0, 0 x NaN = NaN.  One block per entry
// of out[PLANT_BLOCKS], so the blocks spread over the CUs.
#define PLANT_N 64
#define PLANT_BLOCKS 256
__global__ __launch_bounds__(64) void lds_planted_read_kernel(float *out) {
    __shared__ float t[PLANT_N];
    if (threadIdx.x < PLANT_N - 1) t[threadIdx.x] = (float)(threadIdx.x + 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int i = 0; i < PLANT_N - 1; ++i) s += t[i];  // 63 * 64 / 2 = 2016, exact
        const volatile float *stale = &t[PLANT_N - 1];
        out[blockIdx.x] = s + 0.0f * *stale;
    }
}

static int set_max(const void *fn) {
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) == hipSuccess ? 0 : 1;
}

extern "C" {

int lds_fill(uint32_t pattern, int blocks, void *stream) {
    if (blocks <= 0) return 2;
    if (set_max(reinterpret_cast<const void *>(lds_fill_kernel))) return 1;
    lds_fill_kernel<<<blocks, LDS_THREADS, LDS_BYTES, reinterpret_cast<hipStream_t>(stream)>>>(pattern);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// key_out, bad_out: uint32[blocks] on the device; bad_out zeroed by the caller
int lds_probe(uint32_t pattern, int blocks, uint32_t *key_out, uint32_t *bad_out, void *stream) {
    if (blocks <= 0 || !key_out || !bad_out) return 2;
    if (set_max(reinterpret_cast<const void *>(lds_probe_kernel))) return 1;
    lds_probe_kernel<<<blocks, LDS_THREADS, LDS_BYTES, reinterpret_cast<hipStream_t>(stream)>>>(pattern, key_out,
                                                                                                 bad_out);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int lds_planted_blocks(void) { return PLANT_BLOCKS; }

// out: float[PLANT_BLOCKS] on the device; every entry is 2016.0f when the stale word is finite
int lds_planted_read(float *out, void *stream) {
    if (!out) return 2;
    lds_planted_read_kernel<<<PLANT_BLOCKS, 64, 0, reinterpret_cast<hipStream_t>(stream)>>>(out);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // extern "C"
