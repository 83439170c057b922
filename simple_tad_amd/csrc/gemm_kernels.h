// 16-bit-operand (bf16 / f16, see common.h) MFMA GEMMs for the Linear layers of the Video-ViT path (gfx950, wave64).
//
//  gemm_nt : C[M,N] = A[M,K] * B[N,K]^T (+ fused epilogue)      forward Linear and input-gradient (with W^T)
//  gemm_tn : C[N,K] = P[Mr,N]^T * Q[Mr,K]  (split over Mr)        weight gradient
//
// Both stage 64-deep K-tiles global -> LDS with 16-byte LDS-DMA loads (buffer_load ... lds; out-of-range rows
// read as zero through the buffer descriptor's bounds check), double-buffered, one barrier per K-tile, and use
// v_mfma_f32_16x16x32_{bf16,f16}.  The LDS images are XOR-swizzled on the 16-byte chunk index (the swizzle is applied
// to the per-lane *source* address because the DMA destination is lane-linear) so that every ds_read_b128 /
// ds_read_b64_tr_b16 below is bank-conflict free (tools/lds_bank_sim.py).
//
// gemm_nt computes C^T tiles (W rows feed the MFMA "A" operand) with a permuted assignment of W rows to fragment
// lanes, so that each lane ends up holding 4 (f32) or 8 (bf16) *consecutive* output columns of one output row.  Above
// 1.5 tiles per CU it runs persistently (one workgroup per CU walks a tile list and fetches the next tile's first
// K-tile under the current epilogue); the launcher picks the tile shape -- or whole rounds of 256 x 256 tiles plus a
// second launch for the remaining rows -- from a small cost model.  Epilogue (bias / GELU / residual / layer-scale /
// drop-path scale / GELU-backward): accumulators transposed through the LDS so that global accesses cover whole rows,
// raw buffer loads / stores without per-lane branches, what it reads fetched one chunk ahead; bias-only bf16 outputs are
// stored straight from the MFMA layout instead.  DESIGN.md section 3 and docs/DESIGN_HISTORY.md section 3.1 have the measurements behind each choice.
#pragma once
#include "common.h"
#include "gemm_plan.h"  // the epilogue kinds (EPI_*), BK, the plan steps

TAD_NAMESPACE_BEGIN

int launch_reduce_partials(const float* partial, float* out, int splits, int64_t n, int accumulate, hipStream_t st);
int launch_reduce_col_ranges(const float* partial, int N, int splits, int c0, float* out0, int c1, float* out1, int n, int accumulate,
                             hipStream_t st);
int launch_reduce_dw(const float* partial, float* out, int splits, int64_t n, int accumulate, const float* partial2, int rows2, int n2,
                     float* out2a, float* out2b, int n2a, int c2b, hipStream_t st);
int launch_reduce_dw_pair(const float* partial, float* outA, float* outB, int64_t nA, int splits, int64_t n, int accumulate, const float* partial2,
                          int rows2, int n2, float* out2a, float* out2b, int n2a, int c2b, hipStream_t st);

// Ablation switches (TAD_GEMM_DEBUG, see GemmNT::debug) cost scalar branches inside the K loops: compiled in only with
// -DTAD_GEMM_ABLATION (python -m simple_tad_amd.build reads TAD_BUILD_ABLATION=1); production builds see a constant 0.
#ifdef TAD_GEMM_ABLATION
#define DBG_BITS(p) ((p).debug)
#else
#define DBG_BITS(p) 0
#endif

struct GemmNT {
  const uint16_t* A;  // [M,K]
  const uint16_t* B;  // [N,K]
  void* C;            // [M,N] f32 or bf16
  const float* bias;  // [N] or null
  const float* bias2; // with bias_seg > 0: columns [0, seg) take bias[n], [2 seg, 3 seg) take bias2[n - 2 seg], the rest 0 (qkv Linear)
  int bias_seg;
  float colscale;          // EPI_PLAIN: columns [0, colscale_cols) are multiplied by colscale before the one rounding to the output
  int colscale_cols;       // type (0 = off; a multiple of 8).  The q third of the qkv Linear: q * scale * log2(e) (tad_linear_fwd_qkv)
  const float* residual;   // [M or res_mod, N] f32 or null
  const float* gamma;      // [N] or null
  const float* rowscale;   // [ceil(M/rows_per_scale)] or null
  uint16_t* preact;        // [M,N] bf16 or null (EPI_GELU)
  const uint16_t* dgelu_h; // [M,N] bf16 (EPI_DGELU)
  int rows_per_scale;
  int res_mod;  // >0: residual row index = (row_base + m) % res_mod (pos_embed broadcast over the batch)
  int row_base;  // row of the whole problem that this launch's row 0 is (a launch may cover a row range of a Linear): rowscale / res_mod
  int c_bf16;
  int epi;
  int M, N, K;
  int debug;  // ablation (TAD_GEMM_DEBUG, timing only, wrong results): 1 = no DMA inside the K loop, 2 = no MFMA, 4 = no epilogue,
              // 8 = (gemm_tn) no fragment reads and no MFMA: staging and barriers only, 16 = (gemm_tn) unswizzled DMA source
  // split-K launch (SPLITK kernels: the under-filled last round of a Linear, see launch_gemm_nt): every 256 x 256 tile is computed by
  // sk_splits workgroups, each over its share of the K-tiles; sk_ws holds their f32 partial tiles [tile][split][256][256], sk_cnt one
  // arrival counter per tile (zeroed by the launcher), sk_err a word IN PINNED HOST MEMORY that is set if a wait gave up: the host looks at
  // it at the start of every later Linear launch and fails that call loudly (launch_gemm_nt)
  float* sk_ws;
  unsigned* sk_cnt;
  unsigned* sk_err;
  int sk_splits;
  int sk_mode;  // 0: partial tiles combined inside the launch (arrival counters); 1: this launch only leaves the partial tiles (no wait);
                // 2: this launch only combines what a mode-1 launch left (no K loop) -- the "deferred" split-K plan, see launch_gemm_nt
  int group_m;        // tile raster: row panels swept per column panel before moving to the next column panel (L2 reuse)
  unsigned long long* stamps;  // debug timeline (tad_linear_debug_stamps): per workgroup 64 slots of 4 x s_memrealtime, or null
};

int launch_gemm_nt_w4(const GemmNT& p, int grid_persist, hipStream_t st);  // csrc/gemm_w4.hip: the four-wave 256 x 256 kernels
struct GemmTN;
int launch_gemm_tn_w4(const GemmTN& p, int grid, hipStream_t st);

constexpr int ROW_BYTES = BK * 2;  // 128

// swizzle of the 16-byte chunk index (0..7) within a 128-byte LDS row
__device__ __forceinline__ int sw_nt(int row) { return ((row >> 1) & 7) ^ (((row >> 4) & 3) << 1); }

// one wave issues PIECES 1-KiB LDS-DMA pieces: piece i of wave w lands at tile + (i*NW + w)*1024; off[i] is the lane's byte
// offset into the buffer resource (already swizzled), `add` the per-tile advance
// SCALAR_ADD: `add` goes into the instruction's scalar offset instead of a v_add per piece (8 short-lived VGPRs at the point of the
// loop where the fragments are live too: the DGELU / residual 256 x 256 kernels spilled there, and the reload's vmcnt(0) drained the
// DMA).  Only legal when off[i] alone decides whether the access is inside the operand -- true for gemm_nt, whose `add` moves along
// a row (rows >= M have off[i] >= gbytes already), not for gemm_tn, whose `add` moves down the rows -- so the bounds check gives the
// same answer whether or not the hardware includes the scalar offset in it.
template <int PIECES, int NW, bool SCALAR_ADD = false>
__device__ __forceinline__ void stage_tile(const void* gbase, int gbytes, char* tile, const uint32_t* off, uint32_t add, int wave) {
  // descriptor over the whole operand: reads past the end return 0 (rows beyond M / N)
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(gbase), 0, gbytes, 0x00020000);
#pragma unroll
  for (int i = 0; i < PIECES; ++i) {
    if (SCALAR_ADD) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, LDS_PTR(tile + (i * NW + wave) * 1024), 16, off[i], add, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, LDS_PTR(tile + (i * NW + wave) * 1024), 16, off[i] + add, 0, 0, 0);
  }
}

// One 1-KiB LDS-DMA piece of the four-wave kernel (W4 in gemm_nt_kernel): `dst` = LDS address of the piece, `off` = the lane's byte offset
// into the operand (swizzled), `add` = the K-tile's advance along the row (scalar offset: see SCALAR_ADD above).  A function, not a macro
// inside the kernel's nested generic lambdas: with the builtin called there, the HOST pass of hipcc dropped the kernel's launch stub
// without a diagnostic.
__device__ __forceinline__ void w4_dma_piece(const void* gbase, int gbytes, char* dst, uint32_t off, uint32_t add) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(gbase), 0, gbytes, 0x00020000), LDS_PTR(dst), 16, off, add, 0, 0);
}

// wait until at most `stages_in_flight` later stages (LOADS DMA instructions each, per wave) plus EXTRA younger vector-memory
// instructions are still outstanding
template <int LOADS, int EXTRA = 0>
__device__ __forceinline__ void wait_stage(int stages_in_flight) {
  static_assert(3 * LOADS + EXTRA <= 63, "vmcnt immediate is 6 bits");
  if (stages_in_flight >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * LOADS + EXTRA) : "memory");
  else if (stages_in_flight == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LOADS + EXTRA) : "memory");
  else if (stages_in_flight == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LOADS + EXTRA) : "memory");
  else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(EXTRA) : "memory");
}
__device__ __forceinline__ void block_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// barrier between LDS producers and consumers that leaves global stores / loads in flight
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

// PERSIST: one workgroup per CU walks a strided list of tiles (see the comment at the tile loop).
// DIRECT: the epilogue runs on the accumulator registers and stores straight from the MFMA layout (16 rows x 64 contiguous bytes
// per store instruction); otherwise the accumulators are transposed through the LDS first (whole rows per instruction).
// SPLITK: one workgroup = one SHARE of a tile's K-tiles (grid = tiles x p.sk_splits, all of them resident at once: the launcher keeps
// the grid within one workgroup per CU).  The workgroup leaves its f32 partial tile in p.sk_ws, announces it on the tile's arrival
// counter, waits until all shares of the tile are there, and then finishes ITS rows of the tile: sum over the shares, epilogue,
// store.  Nobody waits before publishing, so the wait cannot deadlock while the grid is resident; it is bounded all the same.
// The hand-off follows cdna_hip_programming.md Guideline 16 (plain stores, every wave's vmcnt(0), barrier, one lane's agent-scope
// release, counter add; one relaxed poll, one agent-scope acquire, barrier, plain loads) and depends on no placement.
template <int BM, int BN, int WAVES_M, int WAVES_N, int STAGES, int EPI, bool OUT_BF16, bool PERSIST, bool DIRECT, bool SPLITK = false>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64, 1) void gemm_nt_kernel(const GemmNT p) {
  static_assert(!SPLITK || (!PERSIST && !DIRECT && BM == 256 && BN == 256 && (EPI == EPI_PLAIN || EPI == EPI_RESIDUAL)), "split-K variant");
  constexpr int BKT = BK;
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr bool IS_RES = (EPI == EPI_RESIDUAL || EPI == EPI_RESMOD);
  // W4: FOUR waves, one per SIMD, 128 x 128 outputs each (256 accumulator registers in the AGPR half of the unified file, so this
  // instantiation lives in a translation unit of its own, csrc/gemm_w4.hip, compiled without -amdgpu-mfma-vgpr-form) and a K loop whose
  // order of LDS reads, LDS-DMA pieces and matrix instructions is written out by hand (see W4 below).  Against the 8-wave form a
  // K-tile needs a third fewer LDS fragment bytes per matrix instruction (32 x 16-byte reads per 128 MFMAs instead of 24 per 64).
  constexpr bool W4 = NW == 4 && BM == 256 && BN == 256 && STAGES == 2 && !SPLITK && !DIRECT;
  constexpr int ROWB = BKT * 2;               // bytes per LDS row
  constexpr int RPP = 1024 / ROWB;            // rows per 1-KiB DMA piece
  constexpr int CPR = ROWB / 16;              // 16-byte chunks per row
  constexpr int KSTEPS = BKT / 32;
  constexpr int LOADS = BM / (RPP * NW) + BN / (RPP * NW);
  constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  constexpr int MREP = WTM / 16, NREP = WTN / 16;
  constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB;
  constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
  static_assert(BM % (RPP * NW) == 0 && BN % (RPP * NW) == 0, "tile rows must split into whole DMA pieces per wave");
  // one epilogue chunk: CROWS rows of f32, padded stride.  The persistent kernel keeps ring slot 0 out of the epilogue's way
  // (the next tile's first K-tile lands there meanwhile), so its chunks must fit the LDS behind slot 0.
  constexpr int CROWS = BM < 128 ? BM : BM == 192 ? 64 : (((BN > 128 || (NW == 4 && BM == 256)) && IS_RES && !OUT_BF16) ? 32 : (((PERSIST && BN > 128) || NW == 4) ? 64 : 128));
  constexpr int EPI_OFF = PERSIST ? STAGE_BYTES : 0;
  constexpr int EPI_BYTES = DIRECT ? 0 : CROWS * (BN * 4 + 16);
  constexpr int LDS_BYTES = STAGES * STAGE_BYTES > EPI_OFF + EPI_BYTES ? STAGES * STAGE_BYTES : EPI_OFF + EPI_BYTES;
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
  __shared__ __attribute__((aligned(1024))) char lds[LDS_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;

  // Tile order: the XCD remap gives each XCD (private 4 MiB L2) a contiguous range of logical tile ids; inside that range the
  // ids sweep GROUP_M row-panels for one column-panel before moving to the next column-panel, so the ~32 workgroups that are
  // resident on an XCD at any time touch only GROUP_M A-panels and ~32/GROUP_M W-panels (both stay L2-resident).
  //
  // PERSIST: the grid is one workgroup per CU (a multiple of 8).  Workgroup (xcd = blockIdx & 7, j = blockIdx >> 3) walks the
  // ids first + j, first + j + step, ... of its XCD's range, so at any time the XCD works on ~step consecutive ids as above.
  // What is gained over one launch-scheduled workgroup per tile: the first K-tile of the next tile (with the register-layout
  // epilogue: its whole prologue) is fetched under the epilogue, and no workgroup launch sits between two tiles.
  const int GROUP_M = p.group_m;  // row panels per column-panel group (launch_nt_variant; tad_linear_tuning("group_m"))
  const int tiles_n = (p.N + BN - 1) / BN;
  const int tiles_m = (p.M + BM - 1) / BM;
  const int per_group = GROUP_M * tiles_n;
  int t_cur, t_end, t_step, t_first = 0;
  const int xcd = blockIdx.x & 7;
  if (PERSIST) {
    const int j = blockIdx.x >> 3;
    t_first = xcd_remap(xcd, tiles_m * tiles_n);  // first id of this XCD's range
    t_cur = t_first + j;
    t_end = t_first + (tiles_m * tiles_n >> 3) + ((xcd < ((tiles_m * tiles_n) & 7)) ? 1 : 0);
    t_step = gridDim.x >> 3;
  } else if (SPLITK) {
    // logical id = tile * splits + share: the XCD remap keeps consecutive logical ids -- the shares of one tile -- on one XCD
    // (speed only: the partial tiles then travel through one L2)
    t_cur = xcd_remap(blockIdx.x, gridDim.x) / p.sk_splits;
    t_end = t_cur + 1;
    t_step = 1;
  } else {
    t_cur = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    t_end = t_cur + 1;
    t_step = 1;
  }
  const int sk_share = SPLITK ? xcd_remap(blockIdx.x, gridDim.x) % p.sk_splits : 0;
  int m0, n0;
#define DECODE_TILE(tile)                                  \
  {                                                        \
    const int grp = (tile) / per_group;                    \
    const int first_m = grp * GROUP_M;                     \
    const int gsz = min(tiles_m - first_m, GROUP_M);       \
    const int in_grp = (tile) - grp * per_group;           \
    m0 = (first_m + in_grp % gsz) * BM;                    \
    n0 = (in_grp / gsz) * BN;                              \
  }

  // (debug 128, timing only: A rows 128 bytes further apart than K elements -- the caller over-allocates A -- to see what the row stride costs)
  const uint32_t lda_b = (uint32_t)(p.K * 2) + ((DBG_BITS(p) & 128) ? 128u : 0u);
  const int a_bytes = (int)((int64_t)p.M * lda_b), b_bytes = (int)((int64_t)p.N * p.K * 2);

  // ---- DMA addressing: one wave-instruction fills RPP LDS rows (1 KiB); lane -> (row lane/CPR, physical chunk lane%CPR)
  const int drow = lane / CPR, dchunk = lane % CPR;
  uint32_t a_off[BM / (RPP * NW)], b_off[BN / (RPP * NW)];
#define TILE_OFFSETS()                                                                                                 \
  {                                                                                                                    \
    _Pragma("unroll") for (int i = 0; i < BM / (RPP * NW); ++i) {                                                      \
      const int row = (i * NW + wave) * RPP + drow;                                                                    \
      a_off[i] = (uint32_t)(((DBG_BITS(p) & 64) ? 0 : m0) + row) * lda_b + (uint32_t)((dchunk ^ sw_nt(row)) * 16);  /* (debug 64, timing only: every tile reads the A rows of tile 0 -- A always L2-resident) */ \
    }                                                                                                                  \
    _Pragma("unroll") for (int i = 0; i < BN / (RPP * NW); ++i) {                                                      \
      const int row = (i * NW + wave) * RPP + drow;                                                                    \
      b_off[i] = (uint32_t)(n0 + row) * (uint32_t)(p.K * 2) + (uint32_t)((dchunk ^ sw_nt(row)) * 16);           \
    }                                                                                                                  \
  }
#define STAGE_NT(buf, kt) \
  stage_tile<BM / (RPP * NW), NW, true>(p.A, a_bytes, lds + (buf) * STAGE_BYTES, a_off, (uint32_t)((kt) + kt0) * ROWB, wave); \
  stage_tile<BN / (RPP * NW), NW, true>(p.B, b_bytes, lds + (buf) * STAGE_BYTES + A_BYTES, b_off, (uint32_t)((kt) + kt0) * ROWB, wave)

  // ---- fragment addressing
  const int c = lane & 15, kq = lane >> 4;
  // A-operand rows (output rows m): 16 consecutive rows per m-rep
  uint32_t a_rd[MREP];
  int a_sw[MREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i) {
    const int row = wm * WTM + i * 16 + c;
    a_rd[i] = row * ROWB;
    a_sw[i] = sw_nt(row);
  }
  // B-operand rows (output cols n), permuted so that the 4 lanes (kq = 0..3) that share an output row write one contiguous
  // 64-byte segment per store instruction:
  //   f32 output : fragment j, lane c -> W row 16j + 4*(c>>2) + (c&3)            (lane kq holds cols 16j + 4kq .. +3 : 16 B)
  //   bf16 output: fragment j, lane c -> W row 32*(j>>1) + 8*(c>>2) + 4*(j&1) + (c&3)  (pair (j,j+1): cols 32(j>>1) + 8kq .. +7 : 16 B)
  static_assert(NREP % 2 == 0, "bf16 epilogue pairs n-fragments");
  uint32_t b_rd[NREP];
  int b_sw[NREP];
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    const int rl = OUT_BF16 ? (32 * (j >> 1) + 8 * (c >> 2) + 4 * (j & 1) + (c & 3)) : (16 * j + 4 * (c >> 2) + (c & 3));
    const int row = wn * WTN + rl;
    b_rd[j] = row * ROWB;
    b_sw[j] = sw_nt(row);
  }

  const int nk_all = p.K / BKT;
  const int kt0 = SPLITK ? sk_share * nk_all / p.sk_splits : 0;                       // this workgroup's K-tiles: [kt0, kt0 + nk)
  const int nk = SPLITK ? (p.sk_mode == 2 ? 0 : (sk_share + 1) * nk_all / p.sk_splits - kt0) : nk_all;
#define FRAG_A(dst, base, ks) \
  _Pragma("unroll") for (int i = 0; i < MREP; ++i)  \
      dst[i] = *reinterpret_cast<const op16x8*>((base) + a_rd[i] + ((((KSTEPS > 1 ? 4 * (ks) : 0) + kq) ^ a_sw[i]) << 4))
#define FRAG_B(dst, base, ks) \
  _Pragma("unroll") for (int j = 0; j < NREP; ++j)  \
      dst[j] = *reinterpret_cast<const op16x8*>((base) + b_rd[j] + ((((KSTEPS > 1 ? 4 * (ks) : 0) + kq) ^ b_sw[j]) << 4))
#define MFMA_BLOCK(afr, bfr_)                                                                            \
  if (!(DBG_BITS(p) & 2)) {                                                                                  \
    _Pragma("unroll") for (int i = 0; i < MREP; ++i)                                                     \
        _Pragma("unroll") for (int j = 0; j < NREP; ++j)                                                 \
            acc[i][j] = TAD_MFMA_16x16x32(bfr_[j], afr[i], acc[i][j]);    \
  } else {                                                                                               \
    _Pragma("unroll") for (int i = 0; i < MREP; ++i) asm volatile("" ::"v"(afr[i]));                     \
    _Pragma("unroll") for (int j = 0; j < NREP; ++j) asm volatile("" ::"v"(bfr_[j]));                    \
  }
  const bool late = wave >= NW / 2;  // wave-uniform (scalar branches); the MFMA code is shared by both halves
  // epilogue geometry (see the epilogue below)
  constexpr int MREP_C = CROWS / (16 * WAVES_M);     // m-fragments each wave contributes to a chunk
  constexpr int NCHUNK = MREP / MREP_C;
  constexpr int CSTRIDE = BN * 4 + 16;               // padded row stride (bytes): conflict-free 16-byte writes
  constexpr int CPL = OUT_BF16 ? 8 : 4;              // columns per lane in the row pass (16-byte stores)
  constexpr int LPR = BN / CPL, RPI = 64 / LPR;      // lanes per row, rows per wave-instruction
  constexpr int NR = CROWS / (NW * RPI);             // row-instructions per wave per chunk
  constexpr int BATCH_MAX = (IS_RES && BN > 128) ? 2 : 4;  // rows of LDS reads in flight per lane (register budget: the other chunks' accumulators are live)
  constexpr int BATCH = NR < BATCH_MAX ? NR : BATCH_MAX;
  static_assert(MREP % MREP_C == 0 && MREP_C >= 1 && CROWS % (NW * RPI) == 0 && NR % BATCH == 0, "chunking");
  char* const epi_lds = lds + EPI_OFF;

  DECODE_TILE(t_cur);
  TILE_OFFSETS();
  if (0 < nk) { STAGE_NT(0, 0); }
#ifdef TAD_GEMM_ABLATION
  int stamp_i = 0;
#endif
  bool first_tile = true;
#ifdef TAD_GEMM_ABLATION
// slots 0..15: s_memrealtime (100 MHz) per event; slots 16 + k (k = 0, 1): s_memtime (shader clock) at tile start / K-loop end, so that
// (d memtime / d memrealtime) x 100 MHz is the clock the chip holds INSIDE the K loop (MI355X_MICROARCH.md, DVFS item 6)
#define STAMP(k)                                                                                          \
  if (p.stamps && tid == 0 && stamp_i < 64) {                                                             \
    p.stamps[((size_t)blockIdx.x * 64 + stamp_i) * 32 + (k)] = __builtin_amdgcn_s_memrealtime();          \
    if ((k) < 2) p.stamps[((size_t)blockIdx.x * 64 + stamp_i) * 32 + 16 + (k)] = __builtin_amdgcn_s_memtime(); \
  }
#else
#define STAMP(k) (void)0  // timeline stamps (tad_linear_debug_stamps) exist in ablation builds only
#endif
  for (;;) {
  STAMP(0);
  const int em0 = m0, en0 = n0;  // this tile; (m0, n0) move on to the next one when its first K-tile is prefetched
  const int etile = t_cur;
  const bool qtile = EPI == EPI_PLAIN && p.colscale_cols > 0 && n0 < p.colscale_cols;  // (uniform) see GemmNT::colscale
  bool peeled = false;            // PEEL: this tile's last K-tile carried its epilogue and the next tile's first prefetch
  // Global accesses of the epilogue's row pass are raw buffer loads / stores: rows >= M fall outside the descriptor (loads return
  // 0, stores are dropped), columns >= N get an out-of-range offset explicitly.  No per-lane branches, and the barriers of the
  // epilogue wait for LDS traffic only (lgkmcnt) -- a __syncthreads() would also drain every store issued so far (vmcnt(0)).
  constexpr uint32_t OOB = 0x80000000u;  // >= any descriptor size accepted by the launcher
  constexpr int ST_AUX = 2;  // cache policy of the output stores: nt (streamed), so that the 77-308 MB outputs do not displace the operand panels the
                             // other workgroups of the XCD are re-reading
  constexpr int ESZ = OUT_BF16 ? 2 : 4;
  const uint32_t mn_elems = (uint32_t)p.M * (uint32_t)p.N;
  const auto c_rs = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, (int)(mn_elems * ESZ), 0x00020000);
  const auto pre_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.preact, 0, (int)(mn_elems * 2), 0x00020000);
  const auto h_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.dgelu_h, 0, (int)(mn_elems * 2), 0x00020000);
  const auto res_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.residual, 0, (int)((EPI == EPI_RESMOD ? (uint32_t)p.res_mod * (uint32_t)p.N : mn_elems) * 4), 0x00020000);
  const int col = CPL * (lane % LPR);
  const int n = en0 + col;
  const bool nvalid = n < p.N;
  const bool full = (n + CPL <= p.N);             // N % 4 == 0: a bf16 lane has either 8 or 4 valid columns
  const bool n8 = CPL == 4 || (p.N & 7) == 0;     // uniform: every valid lane is a full lane -> one 16-byte access per row
  // What the epilogue READS besides the accumulators (f32 residual rows / bf16 pre-activation rows) is fetched one chunk ahead:
  // chunk 0 during the last K-tile of the main loop, chunk q + 1 while chunk q is processed.  Fetched on demand, each batch of
  // rows exposed a full HBM latency (4 batches x ~3 us per 256 x 128 f32 tile: longer than that tile's K loop at K = 768).
  constexpr bool HAS_EXTRA = !SPLITK && (IS_RES || EPI == EPI_DGELU);  // (the split-K variant reads them in its combine pass)
  constexpr int EXW = (IS_RES) ? CPL / 4 : 1;
  constexpr int NJ = OUT_BF16 ? NREP / 2 : NREP;  // DIRECT: 16-byte column groups per lane and m-fragment
  u32x4 extra[2][HAS_EXTRA ? (DIRECT ? NJ : NR) : 1][EXW];
  // DIRECT addressing: acc[i][j] of lane (c, kq) = out[em0 + wm*WTM + 16i + c][en0 + wn*WTN + cg(j) .. +3], cg as in the LDS path
#define DIRECT_COL(jj) (en0 + wn * WTN + (OUT_BF16 ? 32 * (jj) + 8 * kq : 16 * (jj) + 4 * kq))
#define ISSUE_EXTRA_D(i, buf)                                                                                           \
  if (HAS_EXTRA && (!IS_RES || p.residual)) {                                                               \
    const int m = em0 + wm * WTM + 16 * (i) + c;                                                                        \
    _Pragma("unroll") for (int jj = 0; jj < NJ; ++jj) {                                                                 \
      const int nn = DIRECT_COL(jj);                                                                                    \
      const bool fulld = nn + CPL <= p.N;                                                                               \
      uint32_t o = nn < p.N ? (uint32_t)m * (uint32_t)p.N + (uint32_t)nn : OOB;                                         \
      if (IS_RES) {                                                                                        \
        if (EPI == EPI_RESMOD) o = (nn < p.N && m < p.M) ? (uint32_t)((m + p.row_base) % p.res_mod) * (uint32_t)p.N + (uint32_t)nn : OOB;  \
        const uint32_t rb = o == OOB ? OOB : o * 4;                                                                     \
        extra[buf][jj][0] = __builtin_amdgcn_raw_buffer_load_b128(res_rs, rb, 0, 0);                                    \
        if (CPL == 8) extra[buf][jj][EXW - 1] = __builtin_amdgcn_raw_buffer_load_b128(res_rs, fulld ? rb + 16 : OOB, 0, 0); \
      } else {                                                                                                          \
        const uint32_t hb = o == OOB ? OOB : o * 2;                                                                     \
        if (CPL == 8) {                                                                                                 \
          if (n8) extra[buf][jj][0] = __builtin_amdgcn_raw_buffer_load_b128(h_rs, hb, 0, 0);                            \
          else {                                                                                                        \
            const u32x2 lo = __builtin_amdgcn_raw_buffer_load_b64(h_rs, hb, 0, 0);                                      \
            const u32x2 hi = __builtin_amdgcn_raw_buffer_load_b64(h_rs, fulld ? hb + 8 : OOB, 0, 0);                    \
            extra[buf][jj][0] = u32x4{lo[0], lo[1], hi[0], hi[1]};                                                      \
          }                                                                                                             \
        } else {                                                                                                        \
          const u32x2 lo = __builtin_amdgcn_raw_buffer_load_b64(h_rs, hb, 0, 0);                                        \
          extra[buf][jj][0] = u32x4{lo[0], lo[1], 0u, 0u};                                                              \
        }                                                                                                               \
      }                                                                                                                 \
    }                                                                                                                   \
  }
#define ISSUE_EXTRA(q, buf)                                                                                             \
  if (HAS_EXTRA && (!IS_RES || p.residual)) {                                                               \
    _Pragma("unroll") for (int r = 0; r < NR; ++r) {                                                                    \
      const int lr = (r * NW + wave) * RPI + lane / LPR;                                                                \
      const int m = em0 + (lr / (16 * MREP_C)) * WTM + 16 * MREP_C * (q) + lr % (16 * MREP_C);                          \
      uint32_t o = nvalid ? (uint32_t)m * (uint32_t)p.N + (uint32_t)n : OOB;                                            \
      if (IS_RES) {                                                                                        \
        if (EPI == EPI_RESMOD) o = (nvalid && m < p.M) ? (uint32_t)((m + p.row_base) % p.res_mod) * (uint32_t)p.N + (uint32_t)n : OOB;     \
        const uint32_t rb = o == OOB ? OOB : o * 4;                                                                     \
        extra[buf][r][0] = __builtin_amdgcn_raw_buffer_load_b128(res_rs, rb, 0, 0);                                     \
        if (CPL == 8) extra[buf][r][EXW - 1] = __builtin_amdgcn_raw_buffer_load_b128(res_rs, full ? rb + 16 : OOB, 0, 0); \
      } else {                                                                                                          \
        const uint32_t hb = o == OOB ? OOB : o * 2;                                                                     \
        if (CPL == 8) {                                                                                                 \
          if (n8) extra[buf][r][0] = __builtin_amdgcn_raw_buffer_load_b128(h_rs, hb, 0, 0);                             \
          else {                                                                                                        \
            const u32x2 lo = __builtin_amdgcn_raw_buffer_load_b64(h_rs, hb, 0, 0);                                      \
            const u32x2 hi = __builtin_amdgcn_raw_buffer_load_b64(h_rs, full ? hb + 8 : OOB, 0, 0);                     \
            extra[buf][r][0] = u32x4{lo[0], lo[1], hi[0], hi[1]};                                                       \
          }                                                                                                             \
        } else {                                                                                                        \
          const u32x2 lo = __builtin_amdgcn_raw_buffer_load_b64(h_rs, hb, 0, 0);                                        \
          extra[buf][r][0] = u32x4{lo[0], lo[1], 0u, 0u};                                                               \
        }                                                                                                               \
      }                                                                                                                 \
    }                                                                                                                   \
  }
  // accumulators start from the bias (a per-column constant = per (j, kq, r) constant in this layout): no bias add later
  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int j = 0; j < NREP; ++j) {
    const int nc = n0 + wn * WTN + (OUT_BF16 ? (32 * (j >> 1) + 8 * kq + 4 * (j & 1)) : (16 * j + 4 * kq));
    f32x4 b4 = f32x4{0.f, 0.f, 0.f, 0.f};
    if (EPI != EPI_DGELU && p.bias && nc < p.N && (!SPLITK || sk_share == 0)) {
      if (EPI == EPI_PLAIN && p.bias_seg > 0) {
        if (nc < p.bias_seg || nc >= 2 * p.bias_seg) {
          const float4 t = *reinterpret_cast<const float4*>(nc < p.bias_seg ? p.bias + nc : p.bias2 + (nc - 2 * p.bias_seg));
          b4 = f32x4{t.x, t.y, t.z, t.w};
        }
      } else {
        const float4 t = *reinterpret_cast<const float4*>(p.bias + nc);
        b4 = f32x4{t.x, t.y, t.z, t.w};
      }
    }
#pragma unroll
    for (int i = 0; i < MREP; ++i) acc[i][j] = b4;
  }
  if constexpr (W4) {
    // ---- W4 K loop.  Per K-tile and wave: 128 MFMAs (16 x 16 x 32) in two halves of 64 -- k-step 0 and k-step 1, each as 8 groups of
    // 8 (one x fragment against the 8 w fragments) -- with two fragment sets: while the matrix pipe works through one k-step the 16
    // fragments of the next one arrive (two 16-byte reads behind every group), so the only place the wave waits for the LDS is a counted
    // wait at the half boundary, by which time the data has had 64 MFMAs to land.  K-tile kt + 2 is requested (two LDS-DMA pieces per
    // group) into the ring slot of K-tile kt during kt's SECOND half, behind the one barrier of the tile: every wave has its k-step-1
    // fragments of that slot in registers by then, and the k-step-0 fragments were taken during the previous tile.  So a piece has a
    // whole tile (about 1.1 us) to arrive, one barrier per K-tile orders everything, and nothing but the half-boundary waits separates
    // two matrix instructions.  Every LDS read is inline asm with an immediate offset (common.h): addresses are 32 lane constants
    // computed once per kernel ([slot][k-step][fragment & 3]; fragment q + 4 lies 8 KiB behind fragment q with the same swizzle).
    // (the ring slot is toggled in the address REGISTERS, one v_xor each per K-tile, and in a scalar for the DMA destination: two copies
    //  of the body selected by a branch make the compiler route the 256 accumulators and the fragments through PHI copies and spill)
    static_assert(STAGE_BYTES == 65536, "slot toggle = bit 16 of the LDS address");
    uint32_t a_ad[2][4], b_ad[2][4];  // [k-step][fragment & 3], pointing into the slot that is being read
    {
      const uint32_t l0 = lds_addr(lds);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          a_ad[ks][q] = l0 + a_rd[q] + (uint32_t)((((4 * ks) + kq) ^ a_sw[q]) << 4);
          b_ad[ks][q] = l0 + (uint32_t)A_BYTES + b_rd[q] + (uint32_t)((((4 * ks) + kq) ^ b_sw[q]) << 4);
        }
    }
    static_assert(MREP == 8 && NREP == 8 && LOADS == 16, "W4 geometry");
    op16x8 fa[2][8], fb[2][8];  // [fragment set = k-step][fragment]
    // one LDS-DMA piece of K-tile kt into the ring slot at byte offset SLOT: pieces 0..7 are x rows, 8..15 w rows (stage_tile's layout).
#define W4_PIECE(SLOT, idx, kt_)                                                                                                          \
  if ((idx) < 8) w4_dma_piece(p.A, a_bytes, lds + (SLOT) + (((idx) & 7) * NW + wave) * 1024, a_off[(idx) & 7], (uint32_t)(kt_) * ROWB);    \
  else w4_dma_piece(p.B, b_bytes, lds + (SLOT) + A_BYTES + (((idx) & 7) * NW + wave) * 1024, b_off[(idx) & 7], (uint32_t)(kt_) * ROWB)
    // K-tile 1 (K-tile 0 is on its way: issued before the loop, or under the previous tile's epilogue); nk >= 2 (the launcher's rule)
    static_for<0, 16>([&](auto ic) { W4_PIECE(STAGE_BYTES, decltype(ic)::value, 1); });
    first_tile = false;
    wait_stage<LOADS>(1);
    block_barrier();
    static_for<0, 8>([&](auto gc) {
      constexpr int g = decltype(gc)::value;
      fb[0][g] = lds_read_b128<op16x8, (g >> 2) * 8192>(b_ad[0][g & 3]);
      fa[0][g] = lds_read_b128<op16x8, (g >> 2) * 8192>(a_ad[0][g & 3]);
    });
    int slot = 0;  // byte offset of the ring slot of K-tile kt
    // NEXT / NEXT2 (compile-time): there is a K-tile kt + 1 / kt + 2.  The steady state is ONE copy of the body inside the loop; the last
    // two K-tiles follow it as straight-line code.
    auto w4_tile = [&](auto NEXTC, auto NEXT2C, int kt) {
      constexpr bool NEXT = decltype(NEXTC)::value, NEXT2 = decltype(NEXT2C)::value;
      // ---- first half: k-step 0 products; the k-step-1 fragments of this slot are requested behind each group
      lds_wait<0>(fb[0][0], fb[0][1], fb[0][2], fb[0][3], fb[0][4], fb[0][5], fb[0][6], fb[0][7]);
      lds_wait<0>(fa[0][0], fa[0][1], fa[0][2], fa[0][3], fa[0][4], fa[0][5], fa[0][6], fa[0][7]);
      static_for<0, 8>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        fb[1][g] = lds_read_b128<op16x8, (g >> 2) * 8192>(b_ad[1][g & 3]);
        fa[1][g] = lds_read_b128<op16x8, (g >> 2) * 8192>(a_ad[1][g & 3]);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] = TAD_MFMA_16x16x32(fb[0][j], fa[0][g], acc[g][j]);
        __builtin_amdgcn_sched_barrier(0);
      });
      // ---- second half: k-step 1 products; K-tile kt + 1 has landed -> its k-step-0 fragments; K-tile kt + 2 requested into this slot
      lds_wait<0>(fb[1][0], fb[1][1], fb[1][2], fb[1][3], fb[1][4], fb[1][5], fb[1][6], fb[1][7]);
      lds_wait<0>(fa[1][0], fa[1][1], fa[1][2], fa[1][3], fa[1][4], fa[1][5], fa[1][6], fa[1][7]);
      if constexpr (NEXT) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        block_barrier();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int q = 0; q < 4; ++q) { a_ad[ks][q] ^= (uint32_t)STAGE_BYTES; b_ad[ks][q] ^= (uint32_t)STAGE_BYTES; }
      }
      static_for<0, 8>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if constexpr (NEXT2) {
          W4_PIECE(slot, 2 * g, kt + 2);
          W4_PIECE(slot, 2 * g + 1, kt + 2);
        }
        if constexpr (NEXT) {
          fb[0][g] = lds_read_b128<op16x8, (g >> 2) * 8192>(b_ad[0][g & 3]);
          fa[0][g] = lds_read_b128<op16x8, (g >> 2) * 8192>(a_ad[0][g & 3]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] = TAD_MFMA_16x16x32(fb[1][j], fa[1][g], acc[g][j]);
        __builtin_amdgcn_sched_barrier(0);
      });
      slot ^= STAGE_BYTES;
    };
    int kt = 0;
    for (; kt + 2 < nk; ++kt) w4_tile(std::true_type{}, std::true_type{}, kt);
    w4_tile(std::true_type{}, std::false_type{}, kt);
    w4_tile(std::false_type{}, std::false_type{}, kt + 1);
    // what the epilogue's first chunk reads besides the accumulators: requested BEHIND the K loop here, not inside its last K-tile as in the
    // eight-wave kernels -- beside two live fragment sets the prefetch registers made the residual / DGELU instantiations spill
    if constexpr (HAS_EXTRA) { ISSUE_EXTRA(0, 0); }
    // (persistent: the address registers must point at slot 0 again for the next tile, whose K-tile 0 lands there)
    if ((nk & 1) == 0) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int q = 0; q < 4; ++q) { a_ad[ks][q] ^= (uint32_t)STAGE_BYTES; b_ad[ks][q] ^= (uint32_t)STAGE_BYTES; }
    }
#undef W4_PIECE
  } else {
    // K-tile 0 is already on its way (issued before the loop, or under the previous tile's epilogue); with the DIRECT epilogue
    // (which leaves the LDS alone) so are the other prologue stages of every tile but the first
    if (!DIRECT || first_tile) {
#pragma unroll
      for (int st = 1; st < STAGES - 1; ++st)
        if (st < nk) { STAGE_NT(st, st); }
    }
    first_tile = false;
    int rd = 0, wr = STAGES - 1;
    // PEEL (persistent 256 x 256 kernel with the register-layout bias-only bf16 epilogue, even number of K-tiles): the last
    // K-tile is taken out of the loop and run row fragment by row fragment -- both k-steps of row i back to back, then the conversion and the
    // two 16-byte stores of row i - 1 while row i's eight MFMAs execute -- so the store epilogue runs beside the last 1/nk of the matrix work
    // instead of behind it; the next tile's first K-tile is requested at the TOP of this K-tile (ring slot 0 was last read one K-tile ago and
    // the barrier that opens this K-tile proves it), and the barrier behind the K loop disappears (the next tile's first barrier orders its DMA
    // into slot 1 behind this tile's last reads).  Measured against the unpeeled build (bit-identical results): qkv forward 202 -> 192 us, the four
    // bias-only shapes of a block 677 -> 660 us, the training step 684.4 -> 686.7 clips/s over three alternating pairs.
    constexpr bool PEEL_OK = PERSIST && DIRECT && EPI == EPI_PLAIN && OUT_BF16 && BM == 256 && BN == 256 && KSTEPS == 2 &&
                             STAGES == 2;
    const bool peel = PEEL_OK && nk >= 2 && (nk & 1) == 0 && !(DBG_BITS(p) & 7);
    peeled = peel;
    const int nk_loop = peel ? nk - 1 : nk;
    for (int kt = 0; kt < nk_loop; ++kt) {
      // tile kt has landed once all but the younger stages' DMAs of this wave are done; the barrier then (a) publishes every
      // wave's part of tile kt and (b) proves all waves finished reading tile kt-1, whose buffer the next DMA overwrites
      wait_stage<LOADS>(min(STAGES - 2, nk - 1 - kt));
      block_barrier();
      if (HAS_EXTRA && kt == nk - 1) {
        if (DIRECT) { ISSUE_EXTRA_D(0, 0); } else { ISSUE_EXTRA(0, 0); }
      }
      const char* sa = lds + rd * STAGE_BYTES;
      const char* sb = sa + A_BYTES;
      const bool more = kt + STAGES - 1 < nk;
      const int wr_now = wr, kt_next = kt + STAGES - 1;
      rd = (rd + 1 == STAGES) ? 0 : rd + 1;
      wr = (wr + 1 == STAGES) ? 0 : wr + 1;
      // Issuing a tile's LDS-DMA pieces blocks the issuing wave for ~100 cycles per piece.  The two waves that share a SIMD
      // (wave w and w + NW/2) therefore issue them at different times: the older half before its first k-step, the younger
      // half between its two k-steps, so the SIMD's matrix pipe always has one wave feeding it.
      const bool dma = more && !(DBG_BITS(p) & 1);
      op16x8 af[MREP], bfr[NREP];
      if (dma && !late) { STAGE_NT(wr_now, kt_next); }
      FRAG_B(bfr, sb, 0);
      FRAG_A(af, sa, 0);
      MFMA_BLOCK(af, bfr);
      if (dma && late) { STAGE_NT(wr_now, kt_next); }
      FRAG_B(bfr, sb, 1);
      FRAG_A(af, sa, 1);
      MFMA_BLOCK(af, bfr);
    }
    if constexpr (PEEL_OK) {
      if (peel) {
        wait_stage<LOADS>(0);
        block_barrier();
        const char* sa = lds + rd * STAGE_BYTES;  // rd == 1 (nk even): slot 0 is free
        const char* sb = sa + A_BYTES;
        if (t_cur + t_step < t_end) {  // the next tile's first K-tile, under this one's MFMAs
          DECODE_TILE(t_cur + t_step);
          TILE_OFFSETS();
          STAGE_NT(0, 0);
        }
        op16x8 b0[NREP], b1[NREP];
        FRAG_B(b0, sb, 0);
        FRAG_B(b1, sb, 1);
        const bool n8p = (p.N & 7) == 0;
        auto store_row = [&](auto ic) {
          constexpr int i = decltype(ic)::value;
          const int m = em0 + wm * WTM + 16 * i + c;
#pragma unroll
          for (int jj = 0; jj < NREP / 2; ++jj) {
            const int nn = en0 + wn * WTN + 32 * jj + 8 * kq;
            const bool fulld = nn + 8 <= p.N;
            const uint32_t o = nn < p.N ? (uint32_t)m * (uint32_t)p.N + (uint32_t)nn : OOB;
            const uint32_t ob = o == OOB ? OOB : o * 2;
            if (qtile) {  // (uniform) a tile with columns of the pre-scaled range: tad_linear_fwd_qkv's q_prescale
              const float cs = nn < p.colscale_cols ? p.colscale : 1.f;
#pragma unroll
              for (int e = 0; e < 4; ++e) { acc[i][2 * jj][e] *= cs; acc[i][2 * jj + 1][e] *= cs; }
            }
            const u32x2 lo = u32x2{pack_op16x2(acc[i][2 * jj][0], acc[i][2 * jj][1]), pack_op16x2(acc[i][2 * jj][2], acc[i][2 * jj][3])};
            const u32x2 hi = u32x2{pack_op16x2(acc[i][2 * jj + 1][0], acc[i][2 * jj + 1][1]), pack_op16x2(acc[i][2 * jj + 1][2], acc[i][2 * jj + 1][3])};
            if (n8p) __builtin_amdgcn_raw_buffer_store_b128(u32x4{lo[0], lo[1], hi[0], hi[1]}, c_rs, ob, 0, ST_AUX);
            else {
              __builtin_amdgcn_raw_buffer_store_b64(lo, c_rs, ob, 0, ST_AUX);
              __builtin_amdgcn_raw_buffer_store_b64(hi, c_rs, fulld ? ob + 8 : OOB, 0, ST_AUX);
            }
          }
        };
        static_for<0, MREP>([&](auto ic) {
          constexpr int i = decltype(ic)::value;
          const op16x8 a0 = *reinterpret_cast<const op16x8*>(sa + a_rd[i] + (((0 + kq) ^ a_sw[i]) << 4));
          const op16x8 a1 = *reinterpret_cast<const op16x8*>(sa + a_rd[i] + (((4 + kq) ^ a_sw[i]) << 4));
#pragma unroll
          for (int j = 0; j < NREP; ++j) acc[i][j] = TAD_MFMA_16x16x32(b0[j], a0, acc[i][j]);
#pragma unroll
          for (int j = 0; j < NREP; ++j) acc[i][j] = TAD_MFMA_16x16x32(b1[j], a1, acc[i][j]);
          if constexpr (i >= 1) {
            store_row(std::integral_constant<int, i - 1>{});
            __builtin_amdgcn_sched_barrier(0);
          }
        });
        store_row(std::integral_constant<int, MREP - 1>{});
      }
    }
  }

  // ---- epilogue.  Straight from the MFMA layout a global access touches 16 rows x 64 bytes per instruction (24.6 B/clk per CU
  // against 70 for whole rows: tools/micro/store_rate.hip), so except for the bias-only bf16 case (DIRECT) the accumulators are
  // transposed through the LDS in chunks of CROWS rows and every global load / store of a wave covers whole contiguous rows
  // (512 B - 1 KiB runs).  The variant (EPI, OUT_BF16) is a template parameter, offsets are 32-bit buffer offsets, the rows read
  // besides the accumulators come one chunk ahead (ISSUE_EXTRA), and the LDS reads of a chunk are batched BATCH rows at a time.
  t_cur += t_step;
  if (!peeled) block_barrier();  // every wave is done with the ring
  const bool has_next = PERSIST && t_cur < t_end;
  STAMP(1);
  if (has_next && !peeled) {
    DECODE_TILE(t_cur);
    TILE_OFFSETS();
    if (0 < nk) { STAGE_NT(0, 0); }
    if (DIRECT) {
#pragma unroll
      for (int st = 1; st < STAGES - 1; ++st)
        if (st < nk) { STAGE_NT(st, st); }
    }
  }
  // Per-row scale (drop-path keep / scale of the row's clip): a 256-row tile lies in at most two groups of rows_per_scale rows
  // (1568 tokens per clip), so the tile takes its one or two scales through scalar loads here.  A per-row global load inside the row
  // pass costs a `s_waitcnt vmcnt(0)` per row -- which on CDNA4 also drains every store and the residual rows fetched ahead.
  // The 256-row tiles are only launched with groups of at least 256 rows (launch_nt_variant) and carry no other path; the 128-row tile
  // keeps the per-row load for shorter groups (tiny problems).
  constexpr bool RS_ALWAYS_TILE = BM >= 256;
  float rs_lo = 1.f, rs_hi = 1.f;
  int rs_split = 0x7fffffff;
  const bool rs_tile = IS_RES && p.rowscale && (RS_ALWAYS_TILE || p.rows_per_scale >= BM);
  if (rs_tile) {
    const int g0 = (em0 + p.row_base) / p.rows_per_scale;
    const int last = (em0 + BM - 1 < p.M ? em0 + BM - 1 : p.M - 1) + p.row_base;
    rs_lo = p.rowscale[g0];
    rs_hi = p.rowscale[last / p.rows_per_scale];
    rs_split = (g0 + 1) * p.rows_per_scale - p.row_base;  // first row (of this launch) in the second group
  }
  if (DIRECT && !peeled && !((DBG_BITS(p) & 4) && p.M > 1)) {
    float gam[CPL];
#pragma unroll
    for (int i = 0; i < MREP; ++i) {
      if (i + 1 < MREP) { ISSUE_EXTRA_D(i + 1, (i + 1) & 1); }
      const int m = em0 + wm * WTM + 16 * i + c;
      float rsc = 1.f;
      if (RS_ALWAYS_TILE || rs_tile) rsc = m < rs_split ? rs_lo : rs_hi;
      else if (IS_RES && p.rowscale && m < p.M) rsc = p.rowscale[(m + p.row_base) / p.rows_per_scale];
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        const int nn = DIRECT_COL(jj);
        const bool fulld = nn + CPL <= p.N;
        const uint32_t o = nn < p.N ? (uint32_t)m * (uint32_t)p.N + (uint32_t)nn : OOB;
        const uint32_t ob = o == OOB ? OOB : o * ESZ;
        float v[CPL];
#pragma unroll
        for (int e = 0; e < CPL; ++e) v[e] = OUT_BF16 ? acc[i][2 * jj + (e >> 2)][e & 3] : acc[i][jj][e & 3];
        if (qtile) {
          const float cs = nn < p.colscale_cols ? p.colscale : 1.f;
#pragma unroll
          for (int e = 0; e < CPL; ++e) v[e] *= cs;
        }
        if (EPI == EPI_GELU) {
          if (p.preact) {
            const uint32_t pb = o == OOB ? OOB : o * 2;
            const u32x2 lo = u32x2{pack_op16x2(v[0], v[1]), pack_op16x2(v[2], v[3])};
            if (CPL == 8) {
              const u32x2 hi = u32x2{pack_op16x2(v[CPL - 4], v[CPL - 3]), pack_op16x2(v[CPL - 2], v[CPL - 1])};
              if (n8) __builtin_amdgcn_raw_buffer_store_b128(u32x4{lo[0], lo[1], hi[0], hi[1]}, pre_rs, pb, 0, ST_AUX);
              else {
                __builtin_amdgcn_raw_buffer_store_b64(lo, pre_rs, pb, 0, ST_AUX);
                __builtin_amdgcn_raw_buffer_store_b64(hi, pre_rs, fulld ? pb + 8 : OOB, 0, ST_AUX);
              }
            } else {
              __builtin_amdgcn_raw_buffer_store_b64(lo, pre_rs, pb, 0, ST_AUX);
            }
          }
          gelu_fast_row<CPL / 2>(v);
        } else if (EPI == EPI_DGELU) {
          const u32x4 hh = extra[i & 1][jj][0];
          const uint32_t hw[4] = {hh[0], hh[1], hh[2], hh[3]};
          gelu_grad_fast_row<CPL / 2>(v, hw);
        } else if (IS_RES) {
          if (p.gamma || p.rowscale) {
#pragma unroll
            for (int e = 0; e < CPL; ++e) gam[e] = (p.gamma && nn < p.N && (e < 4 || fulld)) ? p.gamma[nn + e] : 1.f;
#pragma unroll
            for (int e = 0; e < CPL; ++e) v[e] *= gam[e] * rsc;
          }
          if (p.residual) {
#pragma unroll
            for (int e4 = 0; e4 < CPL / 4; ++e4) {
              const u32x4 rr = extra[i & 1][jj][e4 < EXW ? e4 : 0];
              v[4 * e4 + 0] += __uint_as_float(rr[0]); v[4 * e4 + 1] += __uint_as_float(rr[1]);
              v[4 * e4 + 2] += __uint_as_float(rr[2]); v[4 * e4 + 3] += __uint_as_float(rr[3]);
            }
          }
        }
        if (OUT_BF16) {
          const u32x2 lo = u32x2{pack_op16x2(v[0], v[1]), pack_op16x2(v[2], v[3])};
          const u32x2 hi = u32x2{pack_op16x2(v[CPL - 4], v[CPL - 3]), pack_op16x2(v[CPL - 2], v[CPL - 1])};
          if (n8) __builtin_amdgcn_raw_buffer_store_b128(u32x4{lo[0], lo[1], hi[0], hi[1]}, c_rs, ob, 0, ST_AUX);
          else {
            __builtin_amdgcn_raw_buffer_store_b64(lo, c_rs, ob, 0, ST_AUX);
            __builtin_amdgcn_raw_buffer_store_b64(hi, c_rs, fulld ? ob + 8 : OOB, 0, ST_AUX);
          }
        } else {
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])}, c_rs, ob, 0, ST_AUX);
        }
      }
    }
  }
  if constexpr (SPLITK) {
    // ---- split-K: (1) the partial tile goes to the workspace as whole rows, through the LDS transposition of the ordinary epilogue
    const int S = p.sk_splits;
    float* const part = p.sk_ws + ((size_t)etile * S + sk_share) * (size_t)(BM * BN);
    const auto part_rs = __builtin_amdgcn_make_buffer_rsrc((void*)part, 0, BM * BN * 4, 0x00020000);
    if (p.sk_mode != 2) {
#pragma unroll
    for (int q = 0; q < NCHUNK; ++q) {
#pragma unroll
      for (int ii = 0; ii < MREP_C; ++ii) {
        const int lr = wm * (16 * MREP_C) + ii * 16 + c;
#pragma unroll
        for (int j = 0; j < NREP; ++j) {
          const int cc = wn * WTN + (OUT_BF16 ? (32 * (j >> 1) + 8 * kq + 4 * (j & 1)) : (16 * j + 4 * kq));
          *reinterpret_cast<f32x4*>(epi_lds + lr * CSTRIDE + cc * 4) = acc[q * MREP_C + ii][j];
        }
      }
      lds_barrier();
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int lr = (r * NW + wave) * RPI + lane / LPR;
        const int trow = (lr / (16 * MREP_C)) * WTM + 16 * MREP_C * q + lr % (16 * MREP_C);
#pragma unroll
        for (int e4 = 0; e4 < CPL / 4; ++e4) {
          const u32x4 t = *reinterpret_cast<const u32x4*>(epi_lds + lr * CSTRIDE + col * 4 + 16 * e4);
          // write-through (sc1): the partial tile leaves the XCD's L2 as it is stored, so publishing it needs no agent-scope release
          // (a release fence writes back EVERY dirty line of the L2: 8 us and more with 256 KB freshly written per workgroup).
          // The deferred plan (sk_mode 1) is ordered by the kernel boundary and stores with the ordinary output policy.
          if (p.sk_mode == 0) __builtin_amdgcn_raw_buffer_store_b128(t, part_rs, (uint32_t)((trow * BN + col + 4 * e4) * 4), 0, 16);
          else __builtin_amdgcn_raw_buffer_store_b128(t, part_rs, (uint32_t)((trow * BN + col + 4 * e4) * 4), 0, ST_AUX);
        }
      }
      if (q + 1 < NCHUNK) lds_barrier();
    }
    }
    if (p.sk_mode == 1) break;  // (deferred plan: a later launch combines; the kernel boundary orders the two)
    // ---- (2) publish, wait for the other shares of this tile (Guideline 16, form R1: write-through stores, every storing wave
    // drains them, barrier, ONE lane adds to the counter; ONE relaxed poll, one agent-scope acquire, barrier, then plain loads)
    if (p.sk_mode == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __hip_atomic_fetch_add(p.sk_cnt + etile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      unsigned spins = 0;
      while (__hip_atomic_load(p.sk_cnt + etile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)S) {
        __builtin_amdgcn_s_sleep(4);
        if (++spins > (1u << 22)) {  // (seconds: a share of this tile is not running -- the grid was not resident) give up loudly
          __hip_atomic_store(p.sk_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // (pinned host memory: sk_error_word)
          break;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    }
    // ---- (3) this workgroup's rows of the tile: sum over the shares (share 0 carries the bias), epilogue, store
    float gam[CPL];
#pragma unroll
    for (int e = 0; e < CPL; ++e) gam[e] = (IS_RES && p.gamma && nvalid && (e < 4 || full)) ? p.gamma[n + e] : 1.f;
    const int r0 = sk_share * BM / S, r1 = (sk_share + 1) * BM / S;
    const float* const tile_ws = p.sk_ws + (size_t)etile * S * (size_t)(BM * BN);
    const auto ws_rs = __builtin_amdgcn_make_buffer_rsrc((void*)tile_ws, 0, S * BM * BN * 4, 0x00020000);
    // rows r0 + (it * NW + wave) * RPI + lane / LPR; RB row-instructions per batch so that ~16 partial-tile loads are in flight per
    // lane (one dependent round trip per batch instead of one per row); SS = number of shares as a literal
    auto combine = [&](auto SSC) {
      constexpr int SS = decltype(SSC)::value;
      constexpr int RB = (16 / (SS * (CPL / 4))) > 0 ? (16 / (SS * (CPL / 4))) : 1;
      for (int row0 = r0 + wave * RPI + lane / LPR; row0 - (wave * RPI + lane / LPR) < r1; row0 += RB * NW * RPI) {
        u32x4 pv[RB][SS][CPL / 4], rr[RB][CPL / 4];
        uint32_t off[RB];
#pragma unroll
        for (int b = 0; b < RB; ++b) {
          const int row = row0 + b * NW * RPI;
          const bool live = row < r1;
          const int m = em0 + row;
          off[b] = (live && nvalid) ? (uint32_t)m * (uint32_t)p.N + (uint32_t)n : OOB;
#pragma unroll
          for (int sh = 0; sh < SS; ++sh)
#pragma unroll
            for (int e4 = 0; e4 < CPL / 4; ++e4)
              pv[b][sh][e4] = __builtin_amdgcn_raw_buffer_load_b128(ws_rs, live ? (uint32_t)(((sh * BM + row) * BN + col + 4 * e4) * 4) : OOB, 0, 0);
          if (IS_RES && p.residual) {
            const uint32_t rb = off[b] == OOB ? OOB : off[b] * 4;
            rr[b][0] = __builtin_amdgcn_raw_buffer_load_b128(res_rs, rb, 0, 0);
            if (CPL == 8) rr[b][CPL / 4 - 1] = __builtin_amdgcn_raw_buffer_load_b128(res_rs, full ? rb + 16 : OOB, 0, 0);
          }
        }
#pragma unroll
        for (int b = 0; b < RB; ++b) {
          const int m = em0 + row0 + b * NW * RPI;
          float v[CPL];
#pragma unroll
          for (int e = 0; e < CPL; ++e) v[e] = __uint_as_float(pv[b][0][e >> 2][e & 3]);
#pragma unroll
          for (int sh = 1; sh < SS; ++sh)  // fixed order: share 0 (it carries the bias), 1, 2, ...
#pragma unroll
            for (int e = 0; e < CPL; ++e) v[e] += __uint_as_float(pv[b][sh][e >> 2][e & 3]);
          if (IS_RES) {
            if (p.gamma || p.rowscale) {
              float rsc;
              if (RS_ALWAYS_TILE || rs_tile) rsc = m < rs_split ? rs_lo : rs_hi;
              else rsc = (p.rowscale && m < p.M) ? p.rowscale[(m + p.row_base) / p.rows_per_scale] : 1.f;
#pragma unroll
              for (int e = 0; e < CPL; ++e) v[e] *= gam[e] * rsc;
            }
            if (p.residual) {
#pragma unroll
              for (int e = 0; e < CPL; ++e) v[e] += __uint_as_float(rr[b][e >> 2][e & 3]);
            }
          }
          const uint32_t ob = off[b] == OOB ? OOB : off[b] * ESZ;
          if (OUT_BF16) {
            const u32x2 lo = u32x2{pack_op16x2(v[0], v[1]), pack_op16x2(v[2], v[3])};
            const u32x2 hi = u32x2{pack_op16x2(v[CPL - 4], v[CPL - 3]), pack_op16x2(v[CPL - 2], v[CPL - 1])};
            if (n8) __builtin_amdgcn_raw_buffer_store_b128(u32x4{lo[0], lo[1], hi[0], hi[1]}, c_rs, ob, 0, ST_AUX);
            else {
              __builtin_amdgcn_raw_buffer_store_b64(lo, c_rs, ob, 0, ST_AUX);
              __builtin_amdgcn_raw_buffer_store_b64(hi, c_rs, full ? ob + 8 : OOB, 0, ST_AUX);
            }
          } else {
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])}, c_rs, ob, 0, ST_AUX);
          }
        }
      }
    };
    switch (S) {
      case 2: combine(std::integral_constant<int, 2>{}); break;
      case 3: combine(std::integral_constant<int, 3>{}); break;
      case 4: combine(std::integral_constant<int, 4>{}); break;
      case 5: combine(std::integral_constant<int, 5>{}); break;
      case 6: combine(std::integral_constant<int, 6>{}); break;
      case 7: combine(std::integral_constant<int, 7>{}); break;
      default: combine(std::integral_constant<int, 8>{}); break;
    }
  }
  if (!SPLITK && !DIRECT && !((DBG_BITS(p) & 4) && p.M > 1)) {
  float gam[CPL];
#pragma unroll
  for (int e = 0; e < CPL; ++e) gam[e] = (IS_RES && p.gamma && nvalid && (e < 4 || full)) ? p.gamma[n + e] : 1.f;
  // (1) every wave drops its MREP_C x NREP fragments of chunk qq into the chunk buffer
#define DROP_CHUNK(qq)                                                                                                       \
  _Pragma("unroll") for (int ii = 0; ii < MREP_C; ++ii) {                                                                    \
    const int lr = wm * (16 * MREP_C) + ii * 16 + c;                                                                         \
    _Pragma("unroll") for (int j = 0; j < NREP; ++j) {                                                                       \
      const int cc = wn * WTN + (OUT_BF16 ? (32 * (j >> 1) + 8 * kq + 4 * (j & 1)) : (16 * j + 4 * kq));                     \
      *reinterpret_cast<f32x4*>(epi_lds + lr * CSTRIDE + cc * 4) = acc[(qq) * MREP_C + ii][j]; \
    }                                                                                                                        \
  }
#pragma unroll
  for (int q = 0; q < NCHUNK; ++q) {
    DROP_CHUNK(q);
    lds_barrier();
    if (q < 6) { STAMP(4 + 2 * q); }
    if (q + 1 < NCHUNK) { ISSUE_EXTRA(q + 1, (q + 1) & 1); }
    const char* const epi_rd = epi_lds;
    // (2) row-contiguous pass: local row lr <-> tile row (lr / (16*MREP_C))*WTM + 16*MREP_C*q + lr % (16*MREP_C)
#pragma unroll
    for (int r0 = 0; r0 < NR; r0 += BATCH) {
      float v[BATCH][CPL];
      uint32_t off[BATCH];  // element offset m*N + n, or OOB
#pragma unroll
      for (int b = 0; b < BATCH; ++b) {
        const int lr = ((r0 + b) * NW + wave) * RPI + lane / LPR;
        const int m = em0 + (lr / (16 * MREP_C)) * WTM + 16 * MREP_C * q + lr % (16 * MREP_C);
        off[b] = nvalid ? (uint32_t)m * (uint32_t)p.N + (uint32_t)n : OOB;
#pragma unroll
        for (int e4 = 0; e4 < CPL / 4; ++e4) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(epi_rd + lr * CSTRIDE + col * 4 + 16 * e4);
          v[b][4 * e4 + 0] = t[0]; v[b][4 * e4 + 1] = t[1]; v[b][4 * e4 + 2] = t[2]; v[b][4 * e4 + 3] = t[3];
        }
      }
#pragma unroll
      for (int b = 0; b < BATCH; ++b) {
        const uint32_t ob = off[b] == OOB ? OOB : off[b] * ESZ;  // byte offset into C
        if (qtile) {
          const float cs = n < p.colscale_cols ? p.colscale : 1.f;
#pragma unroll
          for (int e = 0; e < CPL; ++e) v[b][e] *= cs;
        }
        if (EPI == EPI_GELU) {
          if (p.preact) {
            const uint32_t pb = off[b] == OOB ? OOB : off[b] * 2;
            const u32x2 lo = u32x2{pack_op16x2(v[b][0], v[b][1]), pack_op16x2(v[b][2], v[b][3])};
            if (CPL == 8) {
              const u32x2 hi = u32x2{pack_op16x2(v[b][CPL - 4], v[b][CPL - 3]), pack_op16x2(v[b][CPL - 2], v[b][CPL - 1])};
              if (n8) __builtin_amdgcn_raw_buffer_store_b128(u32x4{lo[0], lo[1], hi[0], hi[1]}, pre_rs, pb, 0, ST_AUX);
              else {
                __builtin_amdgcn_raw_buffer_store_b64(lo, pre_rs, pb, 0, ST_AUX);
                __builtin_amdgcn_raw_buffer_store_b64(hi, pre_rs, full ? pb + 8 : OOB, 0, ST_AUX);
              }
            } else {
              __builtin_amdgcn_raw_buffer_store_b64(lo, pre_rs, pb, 0, ST_AUX);
            }
          }
          gelu_fast_row<CPL / 2>(v[b]);
        } else if (EPI == EPI_DGELU) {
          const u32x4 hh = extra[q & 1][r0 + b][0];
          const uint32_t hw[4] = {hh[0], hh[1], hh[2], hh[3]};
          gelu_grad_fast_row<CPL / 2>(v[b], hw);
        } else if (IS_RES) {
          if (p.gamma || p.rowscale) {
            const int lr = ((r0 + b) * NW + wave) * RPI + lane / LPR;
            const int m = em0 + (lr / (16 * MREP_C)) * WTM + 16 * MREP_C * q + lr % (16 * MREP_C);
            float rsc;
            if (RS_ALWAYS_TILE || rs_tile) rsc = m < rs_split ? rs_lo : rs_hi;
            else rsc = (p.rowscale && m < p.M) ? p.rowscale[(m + p.row_base) / p.rows_per_scale] : 1.f;
#pragma unroll
            for (int e = 0; e < CPL; ++e) v[b][e] *= gam[e] * rsc;
          }
          if (p.residual) {
#pragma unroll
            for (int e4 = 0; e4 < CPL / 4; ++e4) {
              const u32x4 rr = extra[q & 1][r0 + b][e4 < EXW ? e4 : 0];
              v[b][4 * e4 + 0] += __uint_as_float(rr[0]); v[b][4 * e4 + 1] += __uint_as_float(rr[1]);
              v[b][4 * e4 + 2] += __uint_as_float(rr[2]); v[b][4 * e4 + 3] += __uint_as_float(rr[3]);
            }
          }
        }
        if (OUT_BF16) {
          const u32x2 lo = u32x2{pack_op16x2(v[b][0], v[b][1]), pack_op16x2(v[b][2], v[b][3])};
          const u32x2 hi = u32x2{pack_op16x2(v[b][CPL - 4], v[b][CPL - 3]), pack_op16x2(v[b][CPL - 2], v[b][CPL - 1])};
          if (n8) __builtin_amdgcn_raw_buffer_store_b128(u32x4{lo[0], lo[1], hi[0], hi[1]}, c_rs, ob, 0, ST_AUX);
          else {
            __builtin_amdgcn_raw_buffer_store_b64(lo, c_rs, ob, 0, ST_AUX);
            __builtin_amdgcn_raw_buffer_store_b64(hi, c_rs, full ? ob + 8 : OOB, 0, ST_AUX);
          }
        } else {
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(v[b][0]), __float_as_uint(v[b][1]), __float_as_uint(v[b][2]), __float_as_uint(v[b][3])},
                                                 c_rs, ob, 0, ST_AUX);
        }
      }
    }
    if (q < 6) { STAMP(5 + 2 * q); }
    if (q + 1 < NCHUNK) lds_barrier();
  }
#undef DROP_CHUNK
  }  // epilogue
  STAMP(2);
#ifdef TAD_GEMM_ABLATION
  if (p.stamps) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(3);
  }
  ++stamp_i;
#endif
  if (!has_next) break;
  if (!DIRECT) lds_barrier();  // epilogue reads of the LDS are done before the next tile's DMAs overwrite it
  }  // tile loop
}

// ------------------------------------------------------------------------------------------------------------
// gemm_tn: slab[s][n][k] = sum_{m in split s} P[m][n] * Q[m][k]
struct GemmTN {
  const uint16_t* P;  // [Mr, N]  (dy)
  const uint16_t* Q;  // [Mr, K]  (x)
  float* slab;        // [splits][N][K]
  float* bias_slab;   // [splits * tiles_k][N] partial column sums of P (bias gradient), or null
  int Mr, N, K;
  int rows_per_split;  // multiple of 64
  int debug;           // ablation bits as in GemmNT
  // PAIR (gemm_tn_w4_kernel only; launch_gemm_tn_pair): TWO weight gradients with the same Mr and K in one launch.  Output rows [0, N1) are
  // P^T Q of the first problem (P [Mr, N1]), rows [N1, N) those of the second (P2 [Mr, N - N1], Q2 [Mr, K]); N1 is a multiple of 256 so that no
  // tile straddles the two, and only the first problem has bias column sums.  N1 = 0: one problem
  const uint16_t* P2;
  const uint16_t* Q2;
  int N1;
};

// swizzle of the 16-byte chunk index within a tile row (rows are >= 256 bytes); changes bits 1..3 only
__device__ __forceinline__ int sw_tn(int row) { return ((row & 3) | ((row >> 1) & 4)) << 1; }

// Transposed 16x16x32 fragments from a [64 reduction rows][row bytes] tile: lane (g = lane>>4, li = lane&15) supplies rows
// 32ks + 8g + (li>>2) (+4 for the second read), columns col0 + 4*(li&3); it receives column col0 + li, reduction rows 32ks + 8g + 0..7.

// PDEEP (the 256 x 256 two-stage configuration): the P and Q halves of a stage live in rings of their own, THREE slots for P and two
// for Q (3 x 32 + 2 x 32 KiB = the whole 160 KiB of LDS), and the P half is requested TWO reduction tiles ahead.  The loop is bound by
// the round trip of a stage's DMA, not by its bytes (staging and barriers alone take 75 % of the kernel's time, docs/DESIGN_HISTORY.md
// section 8): with 96 instead of 64 KiB in flight per CU a first-touch miss has half a tile longer to arrive.  Measured (round 4,
// tools/exp_tn_pdeep.py): bit-identical and NOT faster (four dW shapes 716.4 vs 717.6 us) -- the staging is bound by its rate through
// the DMA path (~37 GB/s per CU), not by latency; kept behind tad_linear_tuning("tn_pdeep"), off.
template <int BM, int BN, int WAVES_M, int WAVES_N, int STAGES, bool PDEEP = false>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void gemm_tn_kernel(const GemmTN p) {
  static_assert(!PDEEP || STAGES == 2, "PDEEP extends the two-stage ring");
  constexpr int BKT = BK;
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  constexpr int MREP = WTM / 16, NREP = WTN / 16;
  constexpr int PROW = BM * 2, QROW = BN * 2;  // bytes per LDS row
  constexpr int KSTEPS = BKT / 32;             // reduction rows per stage: 64 (two k-steps) or 32 (one, deeper ring)
  constexpr int P_BYTES = BKT * PROW, Q_BYTES = BKT * QROW;
  constexpr int STAGE_BYTES = P_BYTES + Q_BYTES;
  constexpr int P_PIECES = P_BYTES / 1024 / NW, Q_PIECES = Q_BYTES / 1024 / NW;
  constexpr int P_LPR = PROW / 16, Q_LPR = QROW / 16;  // lanes (16-B chunks) per row
  static_assert(P_BYTES % (1024 * NW) == 0 && Q_BYTES % (1024 * NW) == 0, "tile must split into 1-KiB DMA pieces per wave");
  static_assert(P_LPR <= 64 && Q_LPR <= 64 && PROW >= 256 && QROW >= 256, "row length");
  constexpr int LOADS = P_PIECES + Q_PIECES;
  constexpr int LDS_BYTES_TN = PDEEP ? 3 * P_BYTES + 2 * Q_BYTES : STAGES * STAGE_BYTES;
  static_assert(LDS_BYTES_TN <= 160 * 1024, "LDS budget");
  __shared__ __attribute__((aligned(1024))) char lds[LDS_BYTES_TN];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;

  // linear id = split * tiles + tile, remapped so that one XCD runs (mostly) one split: the workgroups that stream the same
  // rows of dy / x then share them through that XCD's L2 instead of each fetching them from HBM
  const int tiles_k = (p.K + BN - 1) / BN;
  const int tiles = tiles_k * ((p.N + BM - 1) / BM);
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int split = lin / tiles;
  const int tile = lin - split * tiles;
  const int tn_ = tile / tiles_k, tk_ = tile - tn_ * tiles_k;
  const int n0 = tn_ * BM, k0 = tk_ * BN;
  const int mr0 = split * p.rows_per_split;
  const int nt = p.rows_per_split / BKT;

  const int p_bytes = (int)((int64_t)p.Mr * p.N * 2), q_bytes = (int)((int64_t)p.Mr * p.K * 2);

  // DMA: piece = 1 KiB = (1024/PROW) rows; lane -> row lane / P_LPR, physical chunk lane % P_LPR
  uint32_t p_off[P_PIECES], q_off[Q_PIECES];
#pragma unroll
  for (int i = 0; i < P_PIECES; ++i) {
    const int piece = i * NW + wave;
    const int row = piece * (64 / P_LPR) + lane / P_LPR;
    const int chunk = (lane % P_LPR) ^ ((DBG_BITS(p) & 16) ? 0 : sw_tn(row));  // (debug 16: unswizzled source, timing experiments only)
    // columns beyond N only feed outputs that are never stored; clamp keeps the address inside the row
    int col = n0 + chunk * 8;
    if (col > p.N - 8) col = p.N - 8;
    p_off[i] = (uint32_t)(mr0 + row) * (uint32_t)(p.N * 2) + (uint32_t)(col * 2);
  }
#pragma unroll
  for (int i = 0; i < Q_PIECES; ++i) {
    const int piece = i * NW + wave;
    const int row = piece * (64 / Q_LPR) + lane / Q_LPR;
    const int chunk = (lane % Q_LPR) ^ ((DBG_BITS(p) & 16) ? 0 : sw_tn(row));
    int col = k0 + chunk * 8;
    if (col > p.K - 8) col = p.K - 8;
    q_off[i] = (uint32_t)(mr0 + row) * (uint32_t)(p.K * 2) + (uint32_t)(col * 2);
  }
#define STAGE_TN(buf, t) \
  stage_tile<P_PIECES, NW>(p.P, p_bytes, lds + (buf) * STAGE_BYTES, p_off, (uint32_t)(t) * BKT * (uint32_t)(p.N * 2), wave); \
  stage_tile<Q_PIECES, NW>(p.Q, q_bytes, lds + (buf) * STAGE_BYTES + P_BYTES, q_off, (uint32_t)(t) * BKT * (uint32_t)(p.K * 2), wave)
  // PDEEP: P ring = slots 0..2 at the bottom of the LDS, Q ring = slots 0..1 behind it
#define STAGE_P(slot, t) stage_tile<P_PIECES, NW>(p.P, p_bytes, lds + (slot) * P_BYTES, p_off, (uint32_t)(t) * BKT * (uint32_t)(p.N * 2), wave)
#define STAGE_Q(slot, t) stage_tile<Q_PIECES, NW>(p.Q, q_bytes, lds + 3 * P_BYTES + (slot) * Q_BYTES, q_off, (uint32_t)(t) * BKT * (uint32_t)(p.K * 2), wave)

  // transposed fragment reads: 16-lane group g = lane>>4 covers reduction rows 8g..8g+7 of a 32-deep k-step;
  // lane i = lane&15 of the group supplies row (i>>2) (+4 for the second read), columns c0 + 4*(i&3) .. +3
  const int g = lane >> 4, li = lane & 15;
  // bias gradient = column sums of P = P^T * ones: one extra MFMA per row fragment against an all-ones B operand.  The work is
  // spread evenly (the grid is one workgroup per CU, so any imbalance is pure idle time): the tiles_k workgroups that share a
  // row panel take turns over the reduction tiles (t % tiles_k == own column-panel index), and inside a workgroup the WAVES_N
  // waves that share the same rows split the row fragments (i % WAVES_N == wn).  Partials: bias_slab[split*tiles_k + tk_][N].
  const bool bias_on = (p.bias_slab != nullptr);
  static_assert(MREP % WAVES_N == 0, "bias fragments split across the waves of a row");
  constexpr int BREP = MREP / WAVES_N;
  op16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (op16_t)1.0f;
  f32x4 bacc[BREP];
#pragma unroll
  for (int i = 0; i < BREP; ++i) bacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int i = 0; i < MREP; ++i)
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Fragment reads are inline asm (lds_tr16_b64, common.h): with the builtin the compiler drained the LDS-DMA of the next stage
  // (s_waitcnt vmcnt(0)) in front of the first read after it had been issued, i.e. staging and matrix work ran one after the other.
  // Byte offset of a fragment's first read inside its tile for k-step 0; the second read is 4 rows further, k-step 1 32 rows
  // further (neither changes the swizzle: sw_tn looks at row bits 0, 1 and 3), both as instruction immediates.
  static_assert(NREP == 4, "the waits below are written for four column fragments per wave");
  uint32_t p_rd[MREP], q_rd[NREP];
  {
    const int r0 = 8 * g + (li >> 2);
#pragma unroll
    for (int i = 0; i < MREP; ++i) {
      const int col = wm * WTM + 16 * i + 4 * (li & 3);
      p_rd[i] = (uint32_t)(r0 * PROW + (((col >> 3) ^ sw_tn(r0)) << 4) + (col & 7) * 2);
    }
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      const int col = wn * WTN + 16 * j + 4 * (li & 3);
      q_rd[j] = (uint32_t)(r0 * QROW + (((col >> 3) ^ sw_tn(r0)) << 4) + (col & 7) * 2);
    }
  }
  const uint32_t lds0 = lds_addr(lds);

  if (PDEEP) {
    if (0 < nt) { STAGE_P(0, 0); STAGE_Q(0, 0); }
    if (1 < nt) { STAGE_P(1, 1); }
  } else {
#pragma unroll
    for (int st = 0; st < STAGES - 1; ++st)
      if (st < nt) { STAGE_TN(st, st); }
  }
  int rd = 0, wr = STAGES - 1;
  int p_rdslot = 0, q_rdslot = 0;  // (PDEEP) ring slots of reduction tile t
  for (int t = 0; t < nt; ++t) {
    if (PDEEP) {
      // outstanding, oldest first: P(t), Q(t), P(t+1) -- the first two have to be there, the pieces of P(t+1) may still be in flight
      if (t + 1 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P_PIECES) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      wait_stage<LOADS>(min(STAGES - 2, nt - 1 - t));
    }
    block_barrier();
    const uint32_t st_addr = lds0 + (uint32_t)(rd * STAGE_BYTES);
    const uint32_t p_addr = PDEEP ? lds0 + (uint32_t)(p_rdslot * P_BYTES) : st_addr;
    const uint32_t q_addr = PDEEP ? lds0 + (uint32_t)(3 * P_BYTES + q_rdslot * Q_BYTES) : st_addr;
    constexpr int QIMM = PDEEP ? 0 : P_BYTES;  // where the Q half starts relative to q_addr
    const bool more = PDEEP ? (t + 1 < nt) : (t + STAGES - 1 < nt);
    const bool bias_now = bias_on && (t % tiles_k == tk_);
    const int wr_now = wr, t_next = t + STAGES - 1;
    rd = (rd + 1 == STAGES) ? 0 : rd + 1;
    wr = (wr + 1 == STAGES) ? 0 : wr + 1;
    // (PDEEP) what this tile's DMA point issues: Q(t+1) into the slot Q(t-1) left, then P(t+2) into the slot P(t-1) left -- in that
    // order, so that P(t+2) is the youngest when the next tile waits
    const int q_wrslot = q_rdslot ^ 1, p_wrslot = (p_rdslot == 0) ? 2 : p_rdslot - 1;
    const bool more_p = t + 2 < nt;
    q_rdslot ^= 1;
    p_rdslot = (p_rdslot == 2) ? 0 : p_rdslot + 1;
#define KSTEP_TN(ks) \
  if (!(DBG_BITS(p) & 8)) {                                                                                   \
    s16x4 ql_[NREP], qh_[NREP], pl_[MREP], ph_[MREP];                                                         \
    _Pragma("unroll") for (int j = 0; j < NREP; ++j) {                                                        \
      ql_[j] = lds_tr16_b64<QIMM + (ks) * 32 * QROW>(q_addr + q_rd[j]);                                       \
      qh_[j] = lds_tr16_b64<QIMM + (ks) * 32 * QROW + 4 * QROW>(q_addr + q_rd[j]);                            \
    }                                                                                                         \
    _Pragma("unroll") for (int i = 0; i < MREP; ++i) {                                                        \
      pl_[i] = lds_tr16_b64<(ks) * 32 * PROW>(p_addr + p_rd[i]);                                              \
      ph_[i] = lds_tr16_b64<(ks) * 32 * PROW + 4 * PROW>(p_addr + p_rd[i]);                                   \
    }                                                                                                         \
    /* the four column fragments (8 reads), then one row fragment (2 reads) at a time as its MFMAs come up */ \
    lds_wait<2 * MREP>(ql_[0], qh_[0], ql_[1], qh_[1], ql_[2], qh_[2], ql_[3], qh_[3]);                       \
    op16x8 qf[NREP];                                                                                          \
    _Pragma("unroll") for (int j = 0; j < NREP; ++j) qf[j] = join_tr(ql_[j], qh_[j]);                         \
    static_for<0, MREP>([&](auto ic) {                                                                        \
      constexpr int i = decltype(ic)::value;                                                                  \
      lds_wait<2 * (MREP - 1 - i)>(pl_[i], ph_[i]);                                                           \
      const op16x8 pf = join_tr(pl_[i], ph_[i]);                                                              \
      if (!(DBG_BITS(p) & 2)) {                                                                               \
        _Pragma("unroll") for (int j = 0; j < NREP; ++j)                                                      \
            acc[i][j] = TAD_MFMA_16x16x32(qf[j], pf, acc[i][j]);               \
      } else {                                                                                                \
        asm volatile("" ::"v"(pf));                                                                           \
        _Pragma("unroll") for (int j = 0; j < NREP; ++j) asm volatile("" ::"v"(qf[j]));                       \
      }                                                                                                       \
      if (bias_now && (i % WAVES_N) == wn)                                                                    \
        bacc[i / WAVES_N] = TAD_MFMA_16x16x32(pf, ones, bacc[i / WAVES_N]);    \
    });                                                                                                       \
  }
    const bool late = wave >= NW / 2;  // stagger the DMA issue of the two waves that share a SIMD (see gemm_nt_kernel)
    const bool dma = more && !(DBG_BITS(p) & 1);
    static_assert(KSTEPS == 2, "two 32-deep k-steps per stage");
#define ISSUE_TN()                                             \
  if (PDEEP) {                                                   \
    STAGE_Q(q_wrslot, t + 1);                                    \
    if (more_p) { STAGE_P(p_wrslot, t + 2); }                    \
  } else {                                                       \
    STAGE_TN(wr_now, t_next);                                    \
  }
    if (dma && !late) { ISSUE_TN(); }
    KSTEP_TN(0);
    if (dma && late) { ISSUE_TN(); }
    KSTEP_TN(1);
#undef ISSUE_TN
  }

  if (bias_on && li == 0) {
    float* bo = p.bias_slab + ((int64_t)split * tiles_k + tk_) * p.N;
#pragma unroll
    for (int ib = 0; ib < BREP; ++ib)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wm * WTM + 16 * (ib * WAVES_N + wn) + 4 * g + r;
        if (n < p.N) bo[n] = bacc[ib][r];
      }
  }
  // The Q (k) fragments feed the MFMA's row operand, so D[row = k][col = n]: lane (li, g) holds k = 4g .. 4g+3 of output row
  // n = li -- one 16-byte store per fragment (16 rows x 64 contiguous bytes per instruction) instead of four 4-byte stores.
  // K % 8 == 0, so a group of four k is either wholly inside or wholly outside.
  float* out = p.slab + (int64_t)split * p.N * p.K;
#pragma unroll
  for (int i = 0; i < MREP; ++i) {
    const int n = n0 + wm * WTM + 16 * i + li;
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      const int k = k0 + wn * WTN + 16 * j + 4 * g;
      if (n < p.N && k < p.K)
        *reinterpret_cast<float4*>(out + (int64_t)n * p.K + k) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    }
  }
}

TAD_NAMESPACE_END
