// valu_issue_cost.hip — what one wave64 VALU instruction costs the SIMD, per opcode.
//
// DESIGN §3 budgets the integrate kernels in VALU issue slots of 4 cycles each.  This
// program measures the slots: for each opcode below, every wave runs a loop of
// independent instructions (8 chains, 64 instructions per iteration, no memory access),
// with 1, 2 and 3 waves resident per SIMD (one block of 256 / 512 / 768 threads per CU,
// held to one block by its LDS request).  Reported per opcode and occupancy:
//   ns      SIMD time per wave64 instruction: per SIMD (waves grouped by HW_ID / XCC_ID), from
//           its first wave's start to its last wave's end on the constant-rate counter,
//           over the instructions of its waves; the mean over the SIMDs that hold exactly
//           the intended number of waves (the arbiter serves the oldest wave first, so a
//           wave's own duration says nothing about the SIMD)
//   cyc     the same in shader cycles: ns x the shader clock during that kernel, which is
//           the waves' shader-clock counter against the constant-rate one (when the
//           former is a constant clock as well, ns x the nominal clock)
//   x_fma   ns relative to v_fma_f64's at the same occupancy
// One JSON line on stdout.  Build: hipcc --offload-arch=gfx950 -O3 -o valu_issue_cost
// tools/valu_issue_cost.hip
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

enum Op { ADD_F64, MUL_F64, FMA_F64, RCP_F64, RSQ_F64, CNDMASK_B32, CMP_F64, MUL_F64_SGPR, MUL_F64_MOVLIT, MOV_B32, NOPS };
static const char* const OP_NAME[NOPS] = {"v_add_f64", "v_mul_f64", "v_fma_f64", "v_rcp_f64", "v_rsq_f64",
                                          "v_cndmask_b32", "v_cmp_lt_f64", "v_mul_f64_sgpr_const",
                                          "v_mul_f64_movlit", "v_mov_b32"};
// instructions per asm block (MUL_F64_MOVLIT: two v_mov_b32 per multiply, counted as one unit)
constexpr int CHAINS = 8, REPS = 8;

#define X8 "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
#define U8 "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]), "+v"(u[4]), "+v"(u[5]), "+v"(u[6]), "+v"(u[7])
#define ONE(op, k, post) op " %" #k ", %" #k post "\n"
// "op xk, xk<post>" for each of the 8 chains' own registers
#define EACH8(op, post) \
  ONE(op, 0, post) ONE(op, 1, post) ONE(op, 2, post) ONE(op, 3, post) ONE(op, 4, post) ONE(op, 5, post) ONE(op, 6, post) ONE(op, 7, post)

template <int OP>
__global__ void __launch_bounds__(768) cost_kernel(uint64_t* rec, double* sink, double c, uint64_t mask, int iters) {
  double x[CHAINS];
  uint32_t u[CHAINS];
#pragma unroll
  for (int k = 0; k < CHAINS; ++k) {
    x[k] = 1.0 + (threadIdx.x & 63) * 0x1p-10 + k;
    u[k] = threadIdx.x + k;
  }
  const uint32_t uc = (uint32_t)mask ^ threadIdx.x;
  uint64_t m[CHAINS] = {0, 0, 0, 0, 0, 0, 0, 0};
  __syncthreads();
  const uint64_t w0 = wall_clock64(), c0 = __builtin_readcyclecounter();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int r = 0; r < REPS; ++r) {
      if constexpr (OP == ADD_F64) asm volatile(EACH8("v_add_f64", ", %8") : X8 : "v"(c));
      if constexpr (OP == MUL_F64) asm volatile(EACH8("v_mul_f64", ", %8") : X8 : "v"(c));
      if constexpr (OP == FMA_F64) asm volatile(EACH8("v_fma_f64", ", %8, %8") : X8 : "v"(c));
      if constexpr (OP == RCP_F64) asm volatile(EACH8("v_rcp_f64", "") : X8);
      if constexpr (OP == RSQ_F64) asm volatile(EACH8("v_rsq_f64", "") : X8);
      if constexpr (OP == CNDMASK_B32) asm volatile(EACH8("v_cndmask_b32", ", %8, %9") : U8 : "v"(uc), "s"(mask));
      if constexpr (OP == MUL_F64_SGPR) asm volatile(EACH8("v_mul_f64", ", %8") : X8 : "s"(c));
      if constexpr (OP == MOV_B32) asm volatile(EACH8("v_mov_b32", "") : U8);
      if constexpr (OP == CMP_F64)
        asm volatile("v_cmp_lt_f64 %0, %8, %16\nv_cmp_lt_f64 %1, %9, %16\nv_cmp_lt_f64 %2, %10, %16\n"
                     "v_cmp_lt_f64 %3, %11, %16\nv_cmp_lt_f64 %4, %12, %16\nv_cmp_lt_f64 %5, %13, %16\n"
                     "v_cmp_lt_f64 %6, %14, %16\nv_cmp_lt_f64 %7, %15, %16\n"
                     : "=s"(m[0]), "=s"(m[1]), "=s"(m[2]), "=s"(m[3]), "=s"(m[4]), "=s"(m[5]), "=s"(m[6]), "=s"(m[7])
                     : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "v"(c));
      if constexpr (OP == MUL_F64_MOVLIT) {
        // what the compiler emits for an f64 literal that is no inline constant: the pair
        // is materialised with two v_mov_b32, then used as a VGPR operand
        asm volatile("v_mov_b32 v100, 0x9999999a\nv_mov_b32 v101, 0x3ff19999\nv_mul_f64 %0, %0, v[100:101]"
                     : "+v"(x[r % CHAINS])
                     :
                     : "v100", "v101");
      }
    }
  }
  const uint64_t c1 = __builtin_readcyclecounter(), w1 = wall_clock64();
  double s = 0;
  uint64_t mm = 0;
#pragma unroll
  for (int k = 0; k < CHAINS; ++k) {
    s += x[k] + (double)u[k];
    mm ^= m[k];
  }
  const uint32_t waves = blockDim.x / 64, wave = blockIdx.x * waves + threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) {  // rec[4 wave ..]: start, end, shader-clock ticks, place
    const uint64_t hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));    // HW_REG_HW_ID
    const uint64_t xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));  // HW_REG_XCC_ID
    rec[4 * wave] = w0;
    rec[4 * wave + 1] = w1;
    rec[4 * wave + 2] = c1 - c0;
    rec[4 * wave + 3] = (xcc & 0xf) << 32 | (hw & 0xff30);  // XCC; SE, SH, CU (15:8), SIMD (5:4)
  }
  sink[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s + (double)(mm & 1);
}

#define CHECK(e)                                                                 \
  do {                                                                           \
    hipError_t err_ = (e);                                                       \
    if (err_ != hipSuccess) {                                                    \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(err_)); \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

using Kernel = void (*)(uint64_t*, double*, double, uint64_t, int);
static const Kernel KERNELS[NOPS] = {cost_kernel<ADD_F64>, cost_kernel<MUL_F64>, cost_kernel<FMA_F64>, cost_kernel<RCP_F64>,
                                     cost_kernel<RSQ_F64>, cost_kernel<CNDMASK_B32>, cost_kernel<CMP_F64>,
                                     cost_kernel<MUL_F64_SGPR>, cost_kernel<MUL_F64_MOVLIT>, cost_kernel<MOV_B32>};

int main() {
  hipDeviceProp_t p;
  CHECK(hipGetDeviceProperties(&p, 0));
  int wall_khz = 0;
  CHECK(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, 0));
  if (wall_khz <= 0) wall_khz = 100000;
  const double tick_ns = 1e6 / wall_khz;
  const int blocks = p.multiProcessorCount, iters = 2048;
  constexpr int LDS = 96 * 1024;  // more than half a CU's LDS: one block per CU
  const size_t max_waves = (size_t)blocks * 12, max_threads = (size_t)blocks * 768;
  uint64_t* rec;
  double* sink;
  CHECK(hipMalloc(&rec, max_waves * 4 * sizeof(uint64_t)));
  CHECK(hipMalloc(&sink, max_threads * sizeof(double)));
  std::vector<uint64_t> h(max_waves * 4);
  double ns[NOPS][3], mhz[NOPS][3], share[NOPS][3];
  struct Simd {
    uint64_t t0 = ~0ull, t1 = 0;
    int waves = 0;
  };
  for (int op = 0; op < NOPS; ++op) {
    CHECK(hipFuncSetAttribute((const void*)KERNELS[op], hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    // units per wave and iteration (MUL_F64_MOVLIT: REPS units of mov, mov, mul)
    const double per_wave = (op == MUL_F64_MOVLIT ? REPS : CHAINS * REPS) * (double)iters;
    for (int w = 1; w <= 3; ++w) {
      for (int rep = 0; rep < 2; ++rep) {  // the first launch warms the instruction cache
        hipLaunchKernelGGL(KERNELS[op], dim3(blocks), dim3(256 * w), LDS, 0, rec, sink, 1.0000001, 0x5555555555555555ull, iters);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
      }
      const size_t n = (size_t)blocks * 4 * w;
      CHECK(hipMemcpy(h.data(), rec, n * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
      std::map<uint64_t, Simd> simds;
      double wall_sum = 0, core_sum = 0;
      for (size_t k = 0; k < n; ++k) {
        Simd& s = simds[h[4 * k + 3]];
        if (h[4 * k] < s.t0) s.t0 = h[4 * k];
        if (h[4 * k + 1] > s.t1) s.t1 = h[4 * k + 1];
        ++s.waves;
        wall_sum += (double)(h[4 * k + 1] - h[4 * k]);
        core_sum += (double)h[4 * k + 2];
      }
      double sum = 0;
      int full = 0;
      for (const auto& kv : simds)
        if (kv.second.waves == w) {
          sum += (double)(kv.second.t1 - kv.second.t0) * tick_ns / (per_wave * w);
          ++full;
        }
      ns[op][w - 1] = full ? sum / full : 0.0;
      share[op][w - 1] = (double)full / (double)simds.size();
      mhz[op][w - 1] = core_sum / (wall_sum * tick_ns) * 1e3;
    }
  }
  // the shader-clock counter counts core cycles on some parts and a constant clock on others
  const bool core_is_cycles = mhz[FMA_F64][2] > 500.0;
  const double nominal_mhz = p.clockRate * 1e-3;
  printf("{\"tool\": \"valu_issue_cost\", \"device\": \"%s\", \"cus\": %d, \"nominal_mhz\": %.0f, \"wall_clock_khz\": %d, "
         "\"cycles_from\": \"%s\", \"chains\": %d, \"instructions_per_wave\": %d, \"ops\": {",
         p.gcnArchName, blocks, nominal_mhz, wall_khz, core_is_cycles ? "shader-clock counter" : "ns x nominal clock", CHAINS,
         CHAINS * REPS * iters);
  for (int op = 0; op < NOPS; ++op) {
    printf("%s\"%s\": {", op ? ", " : "", OP_NAME[op]);
    for (int w = 0; w < 3; ++w) {
      const double clk = core_is_cycles ? mhz[op][w] : nominal_mhz;
      printf("%s\"waves%d\": {\"ns\": %.4f, \"cyc\": %.3f, \"x_fma\": %.3f, \"shader_mhz\": %.0f, \"simds_at_occupancy\": %.3f}",
             w ? ", " : "", w + 1, ns[op][w], ns[op][w] * clk * 1e-3, ns[op][w] / ns[FMA_F64][w], clk, share[op][w]);
    }
    printf("}");
  }
  printf("}}\n");
  return 0;
}
