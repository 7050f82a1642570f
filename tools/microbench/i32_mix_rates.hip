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
// Further arms, all in the rows4 shape and on the same registers, each without and with (_LDS) the
// half-step's LDS stream.  Their registers are initialised (the sums stay inside the positive normal
// f32 patterns, as a biased delta row plus an unbiased transition image would) and their maxima
// feed a store:
//   HYB      v_add_u32 + v_max3_f32: exact integer sums, the maximum taken on the same bits as f32
//   HYB_REV  v_add_f32 + v_max3_i32: meaningless, shows which integer instruction breaks co-issue
//   MIX_K16  MIX_K's instructions as 16 adds then 8 max3;  MIX_K32  32 adds then 16 max3
//   MIX_K_I  MIX_K and MIX_LDS built like these arms (registers initialised, the LDS maximum and
//            entry of loop-invariant values, so without MIX_LDS's two v_mov per half-step): the
//            control the other arms are compared with
//   E64      MIX_K with the add in its VOP3 encoding (v_add_u32_e64)
//   LSHL     MIX_K with the add as v_lshl_add_u32 x, d, 0, a
//   SUB, ADD_I32, ADD_CO, ADD3   MIX_K with the add as v_sub_u32, v_add_i32 (VOP3, signed),
//            v_add_co_u32 (carry to vcc), v_add3_u32 x, d, a, 0
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
#define CLOB128 CLOB112, "v112","v113","v114","v115","v116","v117","v118","v119","v120","v121","v122","v123","v124","v125","v126","v127"
#define CLOB ::: CLOB128

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

// the same shape with the instructions named: ADDS4 the four sums of group g, MAXS2 its two maxima
#define ADDS4(ADD, g)                                                          \
  ADD " v[" #g "*16+3], v[" #g "*16+0], v[" #g "*16+1]\n"                      \
  ADD " v[" #g "*16+7], v[" #g "*16+0], v[" #g "*16+2]\n"                      \
  ADD " v[" #g "*16+11], v[" #g "*16+4], v[" #g "*16+5]\n"                     \
  ADD " v[" #g "*16+15], v[" #g "*16+4], v[" #g "*16+6]\n"
#define LSHL4(g)                                                               \
  "v_lshl_add_u32 v[" #g "*16+3], v[" #g "*16+0], 0, v[" #g "*16+1]\n"         \
  "v_lshl_add_u32 v[" #g "*16+7], v[" #g "*16+0], 0, v[" #g "*16+2]\n"         \
  "v_lshl_add_u32 v[" #g "*16+11], v[" #g "*16+4], 0, v[" #g "*16+5]\n"        \
  "v_lshl_add_u32 v[" #g "*16+15], v[" #g "*16+4], 0, v[" #g "*16+6]\n"
// ... for adds with another operand list: PRE x, MID d, a POST
#define ADDS4X(PRE, MID, POST, g)                                                      \
  PRE " v[" #g "*16+3], " MID "v[" #g "*16+0], v[" #g "*16+1]" POST "\n"               \
  PRE " v[" #g "*16+7], " MID "v[" #g "*16+0], v[" #g "*16+2]" POST "\n"               \
  PRE " v[" #g "*16+11], " MID "v[" #g "*16+4], v[" #g "*16+5]" POST "\n"              \
  PRE " v[" #g "*16+15], " MID "v[" #g "*16+4], v[" #g "*16+6]" POST "\n"
#define MAXS2(MAX, g)                                                          \
  MAX " v[" #g "*16+8], v[" #g "*16+8], v[" #g "*16+3], v[" #g "*16+11]\n"     \
  MAX " v[" #g "*16+9], v[" #g "*16+9], v[" #g "*16+7], v[" #g "*16+15]\n"
#define RD2(off, dst)                                                          \
  "ds_read_b128 v[" #dst ":" #dst "+3], %0 offset:" #off "\n"                  \
  "ds_read_b128 v[" #dst "+4:" #dst "+7], %0 offset:" #off "+16\n"
// 8 groups without LDS (48 VALU) and one half-step's four blocks with it (96 VALU), in MIX_K's order
#define BODY(A4, M2) A4(0) M2(0) A4(1) M2(1) A4(2) M2(2) A4(3) M2(3) A4(4) M2(4) A4(5) M2(5) A4(6) M2(6) A4(7) M2(7)
#define BODY_LDS(A4, M2)                                                       \
  RD2(0, 96) A4(0) M2(0) A4(1) M2(1) A4(2) M2(2) A4(3) M2(3)                   \
  RD2(32, 104) A4(4) M2(4) A4(5) M2(5) A4(0) M2(0) A4(1) M2(1)                 \
  RD2(64, 96) A4(2) M2(2) A4(3) M2(3) A4(4) M2(4) A4(5) M2(5)                  \
  RD2(96, 104) A4(0) M2(0) A4(1) M2(1) A4(2) M2(2) A4(3) M2(3)
// ... 16 adds then 8 max3 (one block's worth at a time)
#define BODY16(A4, M2) A4(0) A4(1) A4(2) A4(3) M2(0) M2(1) M2(2) M2(3) A4(4) A4(5) A4(6) A4(7) M2(4) M2(5) M2(6) M2(7)
#define BODY16_LDS(A4, M2)                                                     \
  RD2(0, 96) A4(0) A4(1) A4(2) A4(3) M2(0) M2(1) M2(2) M2(3)                   \
  RD2(32, 104) A4(4) A4(5) A4(0) A4(1) M2(4) M2(5) M2(0) M2(1)                 \
  RD2(64, 96) A4(2) A4(3) A4(4) A4(5) M2(2) M2(3) M2(4) M2(5)                  \
  RD2(96, 104) A4(0) A4(1) A4(2) A4(3) M2(0) M2(1) M2(2) M2(3)
// ... 32 adds then 16 max3 (two blocks' worth; with LDS groups 0 and 1 are summed twice before their
// maxima are taken, which changes no instruction count)
#define BODY32(A4, M2) A4(0) A4(1) A4(2) A4(3) A4(4) A4(5) A4(6) A4(7) M2(0) M2(1) M2(2) M2(3) M2(4) M2(5) M2(6) M2(7)
#define BODY32_LDS(A4, M2)                                                     \
  RD2(0, 96) RD2(32, 104) A4(0) A4(1) A4(2) A4(3) A4(4) A4(5) A4(0) A4(1)      \
  M2(0) M2(1) M2(2) M2(3) M2(4) M2(5) M2(0) M2(1)                              \
  RD2(64, 96) RD2(96, 104) A4(2) A4(3) A4(4) A4(5) A4(0) A4(1) A4(2) A4(3)     \
  M2(2) M2(3) M2(4) M2(5) M2(0) M2(1) M2(2) M2(3)
#define A_U32(g) ADDS4("v_add_u32", g)
#define A_E64(g) ADDS4("v_add_u32_e64", g)
#define A_F32(g) ADDS4("v_add_f32", g)
#define A_SUB(g) ADDS4("v_sub_u32", g)
#define A_I32(g) ADDS4("v_add_i32", g)
#define A_CO(g) ADDS4X("v_add_co_u32", "vcc, ", "", g)
#define A_ADD3(g) ADDS4X("v_add3_u32", "", ", 0", g)
#define M_I32(g) MAXS2("v_max3_i32", g)
#define M_F32(g) MAXS2("v_max3_f32", g)
#define ARM(body) asm volatile(body CLOB)
#define ARM_LDS(body) asm volatile(body : : "v"(rd) : CLOB112, "memory")

// kinds 6 and up come in pairs: even without, odd with the LDS stream
constexpr bool is_lds(int kind) { return kind == 5 || (kind >= 6 && (kind & 1)); }

// 8 independent groups per block; group g uses registers v[16 g + ...] (MIX_LDS: 6 groups)
template <int KIND>
__global__ __launch_bounds__(1024) void k(unsigned long long* cyc, int seed, int* out) {
  __shared__ __attribute__((aligned(16))) int lds[16][8 * 36 + 8];  // per wave: one delta buffer, the maximum
  typedef __attribute__((address_space(3))) int* lds_int_t;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned rd = (unsigned)(size_t)(lds_int_t)&lds[w][(lane & 7) * 36];  // this octet position's rows
  const unsigned wr = (unsigned)(size_t)(lds_int_t)&lds[w][lane];
  const unsigned mx = (unsigned)(size_t)(lds_int_t)&lds[w][8 * 36];
  if (is_lds(KIND)) {
    for (int i = lane; i < 8 * 36 + 8; i += 64) lds[w][i] = seed;
    __syncthreads();
  }
  if constexpr (KIND >= 6) {
    // d = BIAS + v (v_add_f32's arms: a float near 1), the a's, the running maxima at the lowest sum
    const bool rev = KIND == 8 || KIND == 9;
    const int d = rev ? 0x3F800000 - seed * 1000 : 0x7F000000 + seed * 1000;
    const int a1 = rev ? 0x3F000000 - seed * 77 : seed * 77777, a2 = rev ? 0x3E800000 : seed * 3;
    const int m0 = 0x01000000;
#define INIT(groups, clob, ...)                      \
  asm volatile(".irp g, " groups "\n"             \
               "v_mov_b32 v[\\g*16+0], %0\n"      \
               "v_mov_b32 v[\\g*16+4], %0\n"      \
               "v_mov_b32 v[\\g*16+1], %1\n"      \
               "v_mov_b32 v[\\g*16+5], %1\n"      \
               "v_mov_b32 v[\\g*16+2], %2\n"      \
               "v_mov_b32 v[\\g*16+6], %2\n"      \
               "v_mov_b32 v[\\g*16+8], %3\n"      \
               "v_mov_b32 v[\\g*16+9], %3\n"      \
               ".endr"                            \
               :                                  \
               : "s"(d), "s"(a1), "s"(a2), "s"(m0) __VA_ARGS__ \
               : clob)
    if constexpr (is_lds(KIND))
      // the addresses as operands, so they are formed before and not in an initialised register after
      INIT("0,1,2,3,4,5", CLOB112, , "v"(rd), "v"(wr), "v"(mx));
    else
      INIT("0,1,2,3,4,5,6,7", CLOB128);
#undef INIT
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
    } else if constexpr (KIND == 6) {
      ARM(BODY(A_U32, M_F32));
    } else if constexpr (KIND == 7) {
      ARM_LDS(BODY_LDS(A_U32, M_F32));
    } else if constexpr (KIND == 8) {
      ARM(BODY(A_F32, M_I32));
    } else if constexpr (KIND == 9) {
      ARM_LDS(BODY_LDS(A_F32, M_I32));
    } else if constexpr (KIND == 10) {
      ARM(BODY16(A_U32, M_I32));
    } else if constexpr (KIND == 11) {
      ARM_LDS(BODY16_LDS(A_U32, M_I32));
    } else if constexpr (KIND == 12) {
      ARM(BODY32(A_U32, M_I32));
    } else if constexpr (KIND == 13) {
      ARM_LDS(BODY32_LDS(A_U32, M_I32));
    } else if constexpr (KIND == 14) {
      ARM(BODY(A_E64, M_I32));
    } else if constexpr (KIND == 15) {
      ARM_LDS(BODY_LDS(A_E64, M_I32));
    } else if constexpr (KIND == 18) {
      ARM(BODY(A_U32, M_I32));
    } else if constexpr (KIND == 19) {
      ARM_LDS(BODY_LDS(A_U32, M_I32));
    } else if constexpr (KIND == 20) {
      ARM(BODY(A_SUB, M_I32));
    } else if constexpr (KIND == 21) {
      ARM_LDS(BODY_LDS(A_SUB, M_I32));
    } else if constexpr (KIND == 22) {
      ARM(BODY(A_I32, M_I32));
    } else if constexpr (KIND == 23) {
      ARM_LDS(BODY_LDS(A_I32, M_I32));
    } else if constexpr (KIND == 24) {
      asm volatile(BODY(A_CO, M_I32) CLOB, "vcc");
    } else if constexpr (KIND == 25) {
      asm volatile(BODY_LDS(A_CO, M_I32) : : "v"(rd) : CLOB112, "vcc", "memory");
    } else if constexpr (KIND == 26) {
      ARM(BODY(A_ADD3, M_I32));
    } else if constexpr (KIND == 27) {
      ARM_LDS(BODY_LDS(A_ADD3, M_I32));
    } else if constexpr (KIND == 16) {
      ARM(BODY(LSHL4, M_I32));
    } else if constexpr (KIND == 17) {
      ARM_LDS(BODY_LDS(LSHL4, M_I32));
    }
    if constexpr (KIND >= 6 && is_lds(KIND)) {
      // the half-step's maximum and new entry as in MIX_LDS, but of loop-invariant values: a
      // per-iteration v_mov would land in a register the arm has initialised
      if ((lane & 7) == 0) asm volatile("ds_max_i32 %0, %0" : : "v"(mx) : "memory");
      asm volatile("ds_write_b32 %0, %0\n\ts_waitcnt lgkmcnt(0)" : : "v"(wr) : "memory");
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (lane == 0) cyc[blockIdx.x * (blockDim.x >> 6) + w] = t1 - t0;
  if constexpr (KIND >= 6) {  // every group's maxima (the LDS arms have six groups) feed a store
    int r;
    asm volatile(
        "v_xor_b32 %0, v8, v9\n"
        ".irp g, 1,2,3,4,5\n"
        "v_xor_b32 %0, %0, v[\\g*16+8]\n"
        "v_xor_b32 %0, %0, v[\\g*16+9]\n"
        ".endr"
        : "=&v"(r)
        :
        : CLOB112);
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;
  }
}

// VALU instructions per iteration and the (from, to) pairs they cover per lane
constexpr int kInsts[] = {16, 16, 16, 16, 48, 96, 48, 96, 48, 96, 48, 96, 48, 96, 48, 96, 48, 96, 48, 96, 48, 96, 48, 96, 48, 96, 48, 96};
constexpr int kPairs[] = {0, 0, 0, 0, 32, 64, 32, 64, 32, 64, 32, 64, 32, 64, 32, 64, 32, 64, 32, 64, 32, 64, 32, 64, 32, 64, 32, 64};

template <int KIND>
void run(const char* name, int cus) {
  for (int wps : {1, 2, 3, 4}) {
    const int threads = 256 * wps;
    unsigned long long* d;
    int* out;
    (void)hipMalloc(&d, sizeof(unsigned long long) * cus * 16);
    (void)hipMalloc(&out, sizeof(int) * cus * 1024);
    hipLaunchKernelGGL(k<KIND>, dim3(cus), dim3(threads), 0, 0, d, -5, out);
    hipLaunchKernelGGL(k<KIND>, dim3(cus), dim3(threads), 0, 0, d, -5, out);
    (void)hipDeviceSynchronize();
    static unsigned long long h[16 * 1024];
    (void)hipMemcpy(h, d, sizeof(unsigned long long) * cus * (threads / 64), hipMemcpyDeviceToHost);
    double mx = 0;
    for (int i = 0; i < cus * (threads / 64); ++i) mx = h[i] > mx ? (double)h[i] : mx;
    // cycles per VALU instruction per SIMD: all wps waves of a SIMD issue ITERS * kInsts each
    const double cpi = mx / ((double)ITERS * kInsts[KIND] * wps);
    printf("%-11s waves/SIMD %d: %.2f cyc per wave-instruction per SIMD (%.1f lanes/clk/SIMD)", name, wps, cpi, 64 / cpi);
    if (kPairs[KIND]) printf(", %.2f pairs/clk/SIMD", 64.0 * kPairs[KIND] / kInsts[KIND] / cpi);
    printf("\n");
    (void)hipFree(d);
    (void)hipFree(out);
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
  run<18>("MIX_K_I", cus);
  run<19>("MIX_K_I_LDS", cus);
  run<6>("HYB", cus);
  run<7>("HYB_LDS", cus);
  run<8>("HYB_REV", cus);
  run<9>("HYB_REV_LDS", cus);
  run<10>("MIX_K16", cus);
  run<11>("MIX_K16_LDS", cus);
  run<12>("MIX_K32", cus);
  run<13>("MIX_K32_LDS", cus);
  run<14>("E64", cus);
  run<15>("E64_LDS", cus);
  run<16>("LSHL", cus);
  run<17>("LSHL_LDS", cus);
  run<20>("SUB", cus);
  run<21>("SUB_LDS", cus);
  run<22>("ADD_I32", cus);
  run<23>("ADD_I32_LDS", cus);
  run<24>("ADD_CO", cus);
  run<25>("ADD_CO_LDS", cus);
  run<26>("ADD3", cus);
  run<27>("ADD3_LDS", cus);
  return 0;
}
