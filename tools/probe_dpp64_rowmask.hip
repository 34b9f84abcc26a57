// row_mask on 64-bit DPP, gfx950.  The sweep's row rule wants a[rK] = (-pinv) * u on lane row kK only, in ONE instruction; the natural form,
// `v_mul_f64_dpp d, -s0, s1 row_newbcast:N row_mask:M`, does NOT exist: v_mul_f64 (like v_add_f64, v_fma_f64, v_max_f64, v_ldexp_f64) is
// VOP3-only on gfx9 and the assembler rejects it ("dpp variant of this instruction is not supported"); the 64-bit DPP forms are v_fmac_f64
// (the one VOP2 f64 opcode) and the VOP1s (v_mov_b64, v_trunc_f64, ...), all with row_newbcast only.  What can be measured, and is here:
// does `v_fmac_f64_dpp d, -s0, s1 row_newbcast:N row_mask:M bank_mask:0xf` update ONLY the 16-lane rows named in M and leave d on the other
// rows as it was; does it issue at the plain rate; is the two-wait-state rule after a VALU write of the DPP source unchanged
// (tools/probe_dpp64.hip).
// hipcc --offload-arch=gfx950 -O2 -o tools/bin/probe_dpp64_rowmask tools/probe_dpp64_rowmask.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>

#define MULM(N, M) "v_fmac_f64_dpp %[d], -%[s], %[t] row_newbcast:" #N " row_mask:" #M " bank_mask:0xf"

// out[0..63]: d after the masked FMA (7777 + l before it); out[64..127]: fma(-bcast_N(s0), s1, 7777 + l) in plain C++
// out[128..191]: the masked FMA right behind a VALU write of its DPP source, NO nop; out[192..255]: the same behind s_nop 1
// out[256..319]: a plain VALU read of d in the instruction right behind the masked write
template <int N, int M>
__global__ void sem(double* out) {
  const int l = threadIdx.x;
  const double s0 = 1.0 / (l + 3.0), s1 = 0.1 * (l + 7.0);
  double d = 7777.0 + l;
  if (M == 0x1) asm volatile("s_nop 1\n\t" MULM(5, 0x1) : [d] "+v"(d) : [s] "v"(s0), [t] "v"(s1));
  if (M == 0x2) asm volatile("s_nop 1\n\t" MULM(5, 0x2) : [d] "+v"(d) : [s] "v"(s0), [t] "v"(s1));
  if (M == 0x4) asm volatile("s_nop 1\n\t" MULM(5, 0x4) : [d] "+v"(d) : [s] "v"(s0), [t] "v"(s1));
  if (M == 0x8) asm volatile("s_nop 1\n\t" MULM(5, 0x8) : [d] "+v"(d) : [s] "v"(s0), [t] "v"(s1));
  if (M == 0xa) asm volatile("s_nop 1\n\t" MULM(5, 0xa) : [d] "+v"(d) : [s] "v"(s0), [t] "v"(s1));
  if (M == 0xf) asm volatile("s_nop 1\n\t" MULM(5, 0xf) : [d] "+v"(d) : [s] "v"(s0), [t] "v"(s1));
  out[l] = d;
  out[64 + l] = fma(-__shfl(s0, (l & 48) + N), s1, 7777.0 + l);
  double e = l, f = 7777.0 + l, g = 0.0;
  asm volatile("v_add_f64 %[s], %[s], 1.0\n\t" MULM(5, 0x4) "\n\tv_add_f64 %[g], %[d], 0" : [s] "+v"(e), [d] "+v"(f), [g] "+v"(g) : [t] "v"(s1));
  out[128 + l] = f;  // row 2: 7777 + l - (16 row + N + 1) s1 if the hardware interlocks, ... - (16 row + N) s1 if it reads stale
  out[256 + l] = g;  // == f: the masked write is interlocked against a plain read like any VALU write
  double e2 = l, f2 = 7777.0 + l;
  asm volatile("v_add_f64 %[s], %[s], 1.0\n\ts_nop 1\n\t" MULM(5, 0x4) : [s] "+v"(e2), [d] "+v"(f2) : [t] "v"(s1));
  out[192 + l] = f2;
}

template <int FORM>
__global__ void rate(double* out, int iters) {
  double a[16], y = 1.0000001 + threadIdx.x * 1e-12, z = 0.25;
#pragma unroll
  for (int j = 0; j < 16; ++j) a[j] = 1.0 + j + threadIdx.x;
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (FORM == 0) asm volatile("v_fmac_f64 %0, %1, %2" : "+v"(a[j]) : "v"(y), "v"(z));
      if (FORM == 1) asm volatile("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:5 row_mask:0xf bank_mask:0xf" : "+v"(a[j]) : "v"(y), "v"(z));
      if (FORM == 2) asm volatile("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:5 row_mask:0x2 bank_mask:0xf" : "+v"(a[j]) : "v"(y), "v"(z));
      if (FORM == 3) asm volatile("v_mov_b64_dpp %0, %1 row_newbcast:5 row_mask:0x2 bank_mask:0xf" : "+v"(a[j]) : "v"(a[(j + 8) & 15]));
    }
  }
  double s = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) s += a[j];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

static const size_t OUT_DOUBLES = 256ull * 4 * 256;  // the widest rate launch: 1024 blocks x 256 lanes

template <int FORM>
void run(const char* name, double* d) {
  for (int wps : {1, 2, 4}) {
    const int blocks = 256 * wps, iters = 20000;
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(rate<FORM>, dim3(blocks), dim3(256), 0, 0, d, 100);
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL(rate<FORM>, dim3(blocks), dim3(256), 0, 0, d, iters);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    const double ops = (double)blocks * 4 * iters * 16;
    printf("%-44s %d wave/SIMD: %.2f ns per wave-instr per SIMD\n", name, wps, ms * 1e6 / (ops / 1024));
  }
}

template <int M>
int check(double* d) {
  double h[320];
  hipLaunchKernelGGL((sem<5, M>), dim3(1), dim3(64), 0, 0, d);
  if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { printf("row_mask:0x%x : hipMemcpy failed\n", M); return 1; }
  int wrong_written = 0, wrong_kept = 0, stale = 0, bad_nop = 0, bad_read = 0;
  for (int l = 0; l < 64; ++l) {
    const int row = l >> 4;
    if ((M >> row) & 1) wrong_written += memcmp(&h[l], &h[64 + l], 8) != 0;
    else wrong_kept += h[l] != 7777.0 + l;
    const double s1 = 0.1 * (l + 7.0), fresh = fma(-(16.0 * row + 5 + 1), s1, 7777.0 + l), old = fma(-(16.0 * row + 5), s1, 7777.0 + l);
    if (row == 2) {
      stale += h[128 + l] == old && h[128 + l] != fresh;
      bad_nop += h[192 + l] != fresh;
    } else {
      bad_nop += h[192 + l] != 7777.0 + l;
    }
    bad_read += memcmp(&h[256 + l], &h[128 + l], 8) != 0;
  }
  printf("row_mask:0x%x : rows in the mask %s the bits of the plain fma, rows outside %s (lane 5: %.6g, 21: %.6g, 37: %.6g, 53: %.6g)\n", M,
         wrong_written ? "MISS" : "hold", wrong_kept ? "ARE CLOBBERED" : "keep d", h[5], h[21], h[37], h[53]);
  if (M == 0x4)
    printf("hazard, VALU write -> masked DPP read: no nop %s (%d of 16 lanes stale); behind s_nop 1 %s; plain read behind the masked write %s\n",
           stale ? "reads STALE: not interlocked, the two-wait-state rule stands" : "reads fresh", stale, bad_nop ? "WRONG" : "ok",
           bad_read ? "WRONG" : "ok");
  return wrong_written + wrong_kept + bad_nop + bad_read;
}

int main() {
  double* d;
  if (hipMalloc(&d, 8 * OUT_DOUBLES) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
  int bad = check<0x1>(d) + check<0x2>(d) + check<0x4>(d) + check<0x8>(d) + check<0xa>(d) + check<0xf>(d);
  printf("semantics: %s\n", bad ? "MISMATCH" : "ok");
  run<0>("v_fmac_f64 (VOP2)", d);
  run<1>("v_fmac_f64_dpp row_newbcast row_mask:0xf", d);
  run<2>("v_fmac_f64_dpp row_newbcast row_mask:0x2", d);
  run<3>("v_mov_b64_dpp row_newbcast row_mask:0x2", d);
  (void)hipDeviceSynchronize();
  (void)hipFree(d);
  return bad != 0;
}
