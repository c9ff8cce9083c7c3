// Controls for tests/asm_hazards.py, compiled by tests/test_asm_hazards.py into a temporary directory and disassembled there.
// Nothing loads or launches these kernels.  Each hazard sits inside ONE asm string, so it does not depend on the scheduler:
//   ctl_a: an asm load's destination is read before the s_waitcnt that retires it
//   ctl_b: two asm loads, vmcnt(1), then a read of the YOUNGER destination (still in flight)
//   ctl_c: the same with ds_read_b32 and lgkmcnt(1)
//   ctl_*_clean: the same sequences with the read behind a wait that covers it
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" __global__ void ctl_a(const float* p, float* out) {
    float x, y;
    asm volatile("global_load_dword %0, %2, off\n\tv_mov_b32 %1, %0\n\ts_waitcnt vmcnt(0)" : "=&v"(x), "=&v"(y) : "v"(p + threadIdx.x) : "memory");
    out[threadIdx.x] = x + y;
}

extern "C" __global__ void ctl_a_clean(const float* p, float* out) {
    float x, y;
    asm volatile("global_load_dword %0, %2, off\n\ts_waitcnt vmcnt(0)\n\tv_mov_b32 %1, %0" : "=&v"(x), "=&v"(y) : "v"(p + threadIdx.x) : "memory");
    out[threadIdx.x] = x + y;
}

extern "C" __global__ void ctl_b(const float* p, float* out) {
    float x0, x1, y;
    asm volatile("global_load_dword %0, %3, off\n\tglobal_load_dword %1, %3, off offset:4\n\ts_waitcnt vmcnt(1)\n\tv_mov_b32 %2, %1\n\t"
                 "s_waitcnt vmcnt(0)" : "=&v"(x0), "=&v"(x1), "=&v"(y) : "v"(p + threadIdx.x) : "memory");
    out[threadIdx.x] = x0 + x1 + y;
}

extern "C" __global__ void ctl_b_clean(const float* p, float* out) {
    float x0, x1, y;
    asm volatile("global_load_dword %0, %3, off\n\tglobal_load_dword %1, %3, off offset:4\n\ts_waitcnt vmcnt(1)\n\tv_mov_b32 %2, %0\n\t"
                 "s_waitcnt vmcnt(0)" : "=&v"(x0), "=&v"(x1), "=&v"(y) : "v"(p + threadIdx.x) : "memory");
    out[threadIdx.x] = x0 + x1 + y;
}

extern "C" __global__ void ctl_c(float* out) {
    float x0, x1, y;
    const uint32_t a = threadIdx.x * 4u;
    asm volatile("ds_read_b32 %0, %3\n\tds_read_b32 %1, %3 offset:256\n\ts_waitcnt lgkmcnt(1)\n\tv_mov_b32 %2, %1\n\t"
                 "s_waitcnt lgkmcnt(0)" : "=&v"(x0), "=&v"(x1), "=&v"(y) : "v"(a) : "memory");
    out[threadIdx.x] = x0 + x1 + y;
}

extern "C" __global__ void ctl_c_clean(float* out) {
    float x0, x1, y;
    const uint32_t a = threadIdx.x * 4u;
    asm volatile("ds_read_b32 %0, %3\n\tds_read_b32 %1, %3 offset:256\n\ts_waitcnt lgkmcnt(1)\n\tv_mov_b32 %2, %0\n\t"
                 "s_waitcnt lgkmcnt(0)" : "=&v"(x0), "=&v"(x1), "=&v"(y) : "v"(a) : "memory");
    out[threadIdx.x] = x0 + x1 + y;
}
