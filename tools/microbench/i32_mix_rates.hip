// Microbenchmark: gfx950 issue rates of the int32 max-plus instruction mix of trellis_fwd2_i32
// (per two (from, to) pairs: 2 v_add_u32 + 1 v_max3_i32), of its single instructions, and of the
// mix with the kernel's LDS traffic beside it.  Core cycles per wave64 instruction per SIMD from
// s_memtime, at 1 to 4 waves per SIMD (the kernel runs 4: 16 waves of 106 VGPRs per CU).
// The model is f32_mix_rates.hip; registers are named explicitly so every operand's bank (index
// mod 4) is known, and the banks are those of its MIX_K (the kernel's rows4 shape).
//   ADD      v_add_u32 x, d, a                   d, a, x in banks 0, 1, 2
//   MAX3     v_max3_i32 m, m, s0, s1             m, s0, s1 in banks 3, 0, 2
//   MAX2     v_max_i32 m, m, s0                  (VOP2)
//   DPP      v_max_i32_dpp (quad_perm), as the kernel's column fold
//   MIX_K    one d into 2 adds with distinct a's, two rows, then one max3 of 2 sums per column
//   MIX_LDS  MIX_K with the LDS stream of one half-step of the kernel at NP = 256 beside it: per
//            96 VALU instructions 8 ds_read_b128 (two per 8-row block, the lanes of an octet
//            position reading one address), one ds_max_i32 from one lane per octet, one
//            ds_write_b32, and the wait for them at the end.  The adds do not consume what the reads
//            return and the kernel's barrier is not modelled: this is the issue cost of the LDS
//            instructions only, a lower bound of what they cost the kernel
// VALU cycles per instruction count the VALU instructions only, so MIX_LDS against MIX_K is
// what the LDS instructions cost the VALU stream.
#include <hip/hip_runtime.h>

#include <cstdio>

#define ITERS 4096
#define CLOB96 "v0","v1","v2","v3","v4","v5","v6","v7","v8","v9","v10","v11","v12","v13","v14","v15", \
          "v16","v17","v18","v19","v20","v21","v22","v23","v24","v25","v26","v27","v28","v29","v30","v31", \
          "v32","v33","v34","v35","v36","v37","v38","v39","v40","v41","v42","v43","v44","v45","v46","v47", \
          "v48","v49","v50","v51","v52","v53","v54","v55","v56","v57","v58","v59","v60","v61","v62","v63", \
          "v64","v65","v66","v67","v68","v69","v70","v71","v72","v73","v74","v75","v76","v77","v78","v79", \
          "v80","v81","v82","v83","v84","v85","v86","v87","v88","v89","v90","v91","v92","v93","v94","v95"
#define CLOB112 CLOB96, "v96","v97","v98","v99","v100","v101","v102","v103","v104","v105","v106","v107","v108","v109","v110","v111"
#define CLOB ::: CLOB112, "v112","v113","v114","v115","v116","v117","v118","v119","v120","v121","v122","v123","v124","v125","v126","v127"

// the rows4 shape on the registers of group g: 4 adds, 2 max3
#define MIXK(g)                                                                \
  "v_add_u32 v[" #g "*16+3], v[" #g "*16+0], v[" #g "*16+1]\n"                 \
  "v_add_u32 v[" #g "*16+7], v[" #g "*16+0], v[" #g "*16+2]\n"                 \
  "v_add_u32 v[" #g "*16+11], v[" #g "*16+4], v[" #g "*16+5]\n"                \
  "v_add_u32 v[" #g "*16+15], v[" #g "*16+4], v[" #g "*16+6]\n"                \
  "v_max3_i32 v[" #g "*16+8], v[" #g "*16+8], v[" #g "*16+3], v[" #g "*16+11]\n" \
  "v_max3_i32 v[" #g "*16+9], v[" #g "*16+9], v[" #g "*16+7], v[" #g "*16+15]\n"
// one 8-row block of a half-step: its two reads (into v96..v103 / v104..v111), 24 VALU
#define BLOCK(off, dst, g0, g1, g2, g3)                                        \
  "ds_read_b128 v[" #dst ":" #dst "+3], %0 offset:" #off "\n"                  \
  "ds_read_b128 v[" #dst "+4:" #dst "+7], %0 offset:" #off "+16\n" MIXK(g0) MIXK(g1) MIXK(g2) MIXK(g3)

// 8 independent groups per block; group g uses registers v[16 g + ...] (MIX_LDS: 6 groups)
template <int KIND>
__global__ __launch_bounds__(1024) void k(unsigned long long* cyc, int seed) {
  __shared__ __attribute__((aligned(16))) int lds[16][8 * 36 + 8];  // per wave: one delta buffer, the maximum
  typedef __attribute__((address_space(3))) int* lds_int_t;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned rd = (unsigned)(size_t)(lds_int_t)&lds[w][(lane & 7) * 36];  // this octet position's rows
  const unsigned wr = (unsigned)(size_t)(lds_int_t)&lds[w][lane];
  const unsigned mx = (unsigned)(size_t)(lds_int_t)&lds[w][8 * 36];
  if (KIND == 5) {
    for (int i = lane; i < 8 * 36 + 8; i += 64) lds[w][i] = seed;
    __syncthreads();
  }
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < ITERS; ++it) {
    if constexpr (KIND == 0) {  // ADD: x(bank2) = d(bank0) + a(bank1); 16 adds
      asm volatile(
          ".irp g, 0,1,2,3,4,5,6,7\n"
          "v_add_u32 v[\\g*16+2], v[\\g*16+0], v[\\g*16+1]\n"
          "v_add_u32 v[\\g*16+6], v[\\g*16+4], v[\\g*16+5]\n"
          ".endr" CLOB);
    } else if constexpr (KIND == 1) {  // MAX3: m(bank3) = max3(m, s0(bank0), s1(bank2)); 16
      asm volatile(
          ".irp g, 0,1,2,3,4,5,6,7\n"
          "v_max3_i32 v[\\g*16+3], v[\\g*16+3], v[\\g*16+0], v[\\g*16+2]\n"
          "v_max3_i32 v[\\g*16+7], v[\\g*16+7], v[\\g*16+4], v[\\g*16+6]\n"
          ".endr" CLOB);
    } else if constexpr (KIND == 2) {  // MAX2: v_max_i32 m(bank3), m, s0(bank0)
      asm volatile(
          ".irp g, 0,1,2,3,4,5,6,7\n"
          "v_max_i32 v[\\g*16+3], v[\\g*16+3], v[\\g*16+0]\n"
          "v_max_i32 v[\\g*16+7], v[\\g*16+7], v[\\g*16+4]\n"
          ".endr" CLOB);
    } else if constexpr (KIND == 3) {  // DPP: v_max_i32_dpp (quad_perm), 16 independent
      asm volatile(
          ".irp g, 0,1,2,3,4,5,6,7\n"
          "v_max_i32_dpp v[\\g*16+3], v[\\g*16+0], v[\\g*16+3] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
          "v_max_i32_dpp v[\\g*16+7], v[\\g*16+4], v[\\g*16+7] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
          ".endr" CLOB);
    } else if constexpr (KIND == 4) {  // MIX_K: 8 groups of 4 adds + 2 max3
      asm volatile(MIXK(0) MIXK(1) MIXK(2) MIXK(3) MIXK(4) MIXK(5) MIXK(6) MIXK(7) CLOB);
    } else if constexpr (KIND == 5) {  // MIX_LDS: one half-step's four blocks, then the maximum and the new entry
      asm volatile(BLOCK(0, 96, 0, 1, 2, 3) BLOCK(32, 104, 4, 5, 0, 1) BLOCK(64, 96, 2, 3, 4, 5) BLOCK(96, 104, 0, 1, 2, 3)
                   :
                   : "v"(rd)
                   : CLOB112, "memory");
      if ((lane & 7) == 0) asm volatile("ds_max_i32 %0, %1" : : "v"(mx), "v"(it) : "memory");
      asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(wr), "v"(it) : "memory");
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (lane == 0) cyc[blockIdx.x * (blockDim.x >> 6) + w] = t1 - t0;
}

// VALU instructions per iteration and the (from, to) pairs they cover per lane
constexpr int kInsts[] = {16, 16, 16, 16, 48, 96};
constexpr int kPairs[] = {0, 0, 0, 0, 32, 64};

template <int KIND>
void run(const char* name, int cus) {
  for (int wps : {1, 2, 3, 4}) {
    const int threads = 256 * wps;
    unsigned long long* d;
    (void)hipMalloc(&d, sizeof(unsigned long long) * cus * 16);
    hipLaunchKernelGGL(k<KIND>, dim3(cus), dim3(threads), 0, 0, d, -5);
    hipLaunchKernelGGL(k<KIND>, dim3(cus), dim3(threads), 0, 0, d, -5);
    (void)hipDeviceSynchronize();
    static unsigned long long h[16 * 1024];
    (void)hipMemcpy(h, d, sizeof(unsigned long long) * cus * (threads / 64), hipMemcpyDeviceToHost);
    double mx = 0;
    for (int i = 0; i < cus * (threads / 64); ++i) mx = h[i] > mx ? (double)h[i] : mx;
    // cycles per VALU instruction per SIMD: all wps waves of a SIMD issue ITERS * kInsts each
    const double cpi = mx / ((double)ITERS * kInsts[KIND] * wps);
    printf("%-8s waves/SIMD %d: %.2f cyc per wave-instruction per SIMD (%.1f lanes/clk/SIMD)", name, wps, cpi, 64 / cpi);
    if (kPairs[KIND]) printf(", %.2f pairs/clk/SIMD", 64.0 * kPairs[KIND] / kInsts[KIND] / cpi);
    printf("\n");
    (void)hipFree(d);
  }
}

int main() {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, 0) != hipSuccess) return 1;
  const int cus = p.multiProcessorCount;
  if (cus <= 0 || cus > 1024) return 1;
  printf("device %s CUs %d\n", p.gcnArchName, cus);
  run<0>("ADD", cus);
  run<1>("MAX3", cus);
  run<2>("MAX2", cus);
  run<3>("DPP", cus);
  run<4>("MIX_K", cus);
  run<5>("MIX_LDS", cus);
  return 0;
}
