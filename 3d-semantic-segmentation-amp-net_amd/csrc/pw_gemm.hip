// pw_gemm.hip -- the shared per-point MLP layer (Conv1d k=1 / Linear) on the fp32 matrix cores.
//
// Reference ops covered (pointNet/model/pointnetAtt.py): every conv_k / fc_k with K >= 64 of
// TransformationNet (:31-40), BasePointNet (:90-103, and the two torch.bmm at :85/:96 as per-window weights)
// and SegmentationWithAttention (:203-207), each with the PREVIOUS layer's BatchNorm+ReLU(+Dropout) fused as
// a prologue on the A operand and THIS layer's BatchNorm statistics / MaxPool1d fused as epilogue reductions.
//
// CDNA4 mapping
//   * v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD = the fp32 matrix peak).  A wave owns a
//     32-row x (32*NT)-column output tile: NT accumulators of 16 VGPRs.
//   * MFMA "A" = activations (rows = points), "B" = weights, so the accumulator has the OUTPUT CHANNEL on
//     the lane and 16 rows in registers: per-channel sums / max / argmax are in-lane reductions, and a store
//     instruction writes two full 128-byte row segments.
//   * K permutation: lane (r, h) loads 16 bytes A[row r][8j + 4h .. +3] straight from HBM/L2 into registers
//     and feeds them to four consecutive MFMAs; the weight fragment W[col][8j + 4h .. +3] comes from LDS
//     with one ds_read_b128 (row stride CIN + 4 floats: conflict-free).  The MFMA sums over k in a permuted
//     order, both operands agree on it.
//   * weights (<= 128 x 256 fp32 = 133 KB) are staged in LDS once per workgroup and reused for every row tile
//     of the workgroup's chunk; A fragments are prefetched one 128-byte line per row ahead of the MFMAs.
#include <cstdlib>
#include <type_traits>
#include "kernels.h"

namespace ampnet {

constexpr int PW_NW = 4;   // waves per workgroup

// Development probe (tools/x3_stamps.py; built only with -DAMPNET_PW_STAMPS): wave 0 of workgroup 0 of a split kernel records
// (label, s_memtime) pairs into a device buffer -- where a wave's time goes, by phase.
#ifdef AMPNET_PW_STAMPS
__device__ unsigned long long g_pw_stamps[4096];
#define PW_STAMP(id)                                                                                        \
    do {                                                                                                    \
        if (blockIdx.x == 0 && threadIdx.x == 0 && stamp_n < 4000)                                          \
            g_pw_stamps[1 + stamp_n++] = ((unsigned long long)(id) << 48) | (__builtin_readcyclecounter() & 0xffffffffffffull); \
    } while (0)
#else
#define PW_STAMP(id) do { } while (0)
#endif

// 1 / x for x >= 1 to ~1e-16 relative: hardware estimate + two Newton steps (x0 (2 - d x0))
__device__ __forceinline__ double rcp_f64(double d)
{
    double x = __builtin_amdgcn_rcp(d);
    x = x * __builtin_fma(-d, x, 2.0);
    x = x * __builtin_fma(-d, x, 2.0);
    return x;
}

// PRO: prologue on the A operand -- 0 none, 1 relu(a * scale + shift), 2 the same then dropout.  POOL: track the per-channel
// extreme (+ its row) instead of / besides storing.  Both are compile-time so that the K loop and the epilogue are straight-line
// code: LDS reads get scheduled ahead of the MFMAs that use them and no branch sits between two epilogue elements.
// BF: the MFMA operands are rounded to bf16 (activations after the prologue, weights while staged) and multiplied on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- 16 x the fp32 matrix rate; HBM tensors, BatchNorm statistics, the
// prologue and the epilogue stay fp32 (ampnet_set_matrix_precision).  Lane (r, h) then owns k = 16 s + 8 h .. + 7 of step s.
// ABF / ZBF (BF kernels only): A / Z are bf16 tensors (activation storage of precision mode 3); compile-time so that the K loop
// stays one basic block (as a run-time flag the bf16 kernels ran 10-35 % slower).
// PIPE (fp32 path, the default; AMPNET_PW_PIPE=0 turns it off): the operands of a k step are read / computed one step ahead under the MFMAs of the
// current step (tools/ab_pw_pipe.py compares the two forms on one box in one process).
// ARG (pool epilogue only): also track the ROW of the extreme (the backward needs it; an eval forward does not -- one v_max per element instead
// of a compare and two selects)
// X3 (BF kernels, fp32 tensors; precision mode AMPNET_PRECISION_F32_SPLIT): fp32 products from the bf16 pipe -- both operands are split into three
// bf16 terms (the weights once, while staged: three LDS images; the activations after the prologue, in registers, shared by the NT column
// tiles) and a k step issues the six partial products a1 b1, a1 b2, a2 b1, a1 b3, a2 b2, a3 b1 per tile (each exact in fp32; the dropped
// a2 b3 + a3 b2 + a3 b3 is below 2^-23 |a b|): 6 / 16 of the fp32 MFMA time.  NW = waves per workgroup.
template <int CIN, int NT, int PRO, bool POOL, bool BF, bool ABF = false, bool ZBF = false, bool PIPE = false, bool ARG = true, bool X3 = false, int NW = PW_NW, int XRT = 1>
__global__ __launch_bounds__(NW * 64, X3 ? 1 : 2) void pw_gemm_kernel(PwGemm a)
{
    static_assert(!X3 || (BF && !ABF && !ZBF && !PIPE), "the split kernels are bf16-MFMA kernels on fp32 tensors");
    constexpr int PW_NW = NW;          // (shadows the namespace constant: every use below means this kernel's wave count)
    constexpr int NIMG = X3 ? 3 : 1;   // bf16 images of the weight tile in LDS
    // (kernels.h: ld_stream / st_stream -- the switch is kept for the A/B)
    // measured, same box: the FORWARD layers lose 6 .. 20 % with streamed stores (a layer's output is the next layer's input within microseconds and the
    // infinity cache holds a good part of it) and 5 .. 21 % with streamed loads alone (a lane reads 16 bytes of a row per k step: the eight pieces of a
    // 128-byte line arrive over eight instructions, and a line marked evict-first does not survive that long) -- the fused backward, whose staging
    // threads read whole rows per instruction, gains 2 .. 7 % from both (kernels.h)
    constexpr bool STREAM_LD = false, STREAM = false;
    constexpr int CB = 32 * NT;
    constexpr int LDW = CIN + 4;       // fp32 weight row (floats)
    constexpr int LDB = CIN + 8;       // bf16 weight row (elements): 16-byte aligned rows, conflict-free ds_read_b128
    constexpr int NBLK = CIN / 32;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sW = smem;                  // fp32: [CB][LDW]
    __bf16 *sWb = reinterpret_cast<__bf16 *>(smem);   // bf16: [CB][LDB]
    float *sPro = BF ? smem + NIMG * CB * LDB / 2 : smem + CB * LDW;     // scale[CIN], shift[CIN]
    float *sRed = sPro + 2 * CIN;                                  // cross-wave reduction scratch (the weights stay resident)
    double *sRun = reinterpret_cast<double *>(sRed + PW_NW * CB * 5 + PW_NW);   // [CB][2] per-workgroup running (mean, M2): a.part_rows mode

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r = lane & 31;
    const int h = lane >> 5;
    // Persistent workgroups: workgroup (lane, column block) walks the blocks of rows rb = lane, lane + G, ... with the SAME weight
    // tile resident in LDS (staged once, not once per 512 rows).  XCD-aware order: workgroups are dealt round-robin to the
    // 8 XCDs (own L2 each), so the column blocks of one lane get ids 8 apart -- same XCD, same rows at the same time: the
    // second read of those rows hits that L2.
    const int ncb = (a.cout + CB - 1) / CB;
    const int within = blockIdx.x % (8 * ncb);
    const int lane_id = (blockIdx.x / (8 * ncb)) * 8 + within % 8;
    const int n_lanes = (gridDim.x / (8 * ncb)) * 8;
    const int n_rb = a.Q * a.chunks;
    const int cb0 = (within / 8) * CB;
    const bool perwin_w = a.w_win_stride != 0;
    // Statistics per WORKGROUP (a.part_rows != nullptr; the pooled layers too -- their per-(window, chunk) extremes keep their own slots): lane = (slot, j) = (lane_id % n_slots,
    // lane_id / n_slots) walks the blocks of rows j, j + L_slot, ... of ITS slot only (L_slot = the lanes that slot has: stat_lanes / n_slots,
    // one more for the first stat_lanes % n_slots slots), merges their (rows, mean, M2) as it goes and leaves ONE partial per column: ~57
    // partials per slot for bn_finalize (one stage) instead of one per block of rows (two stages) -- or none at all when a slot is a single
    // block of rows (the T-Net FC layers): then the BatchNorm constants are finished right here (PwGemm.fin).  With stat_lanes = the resident
    // grid the blocks of rows are dealt exactly as evenly as by the slot-blind walk (2304 blocks over 512 lanes: 256 lanes take five, 256 four,
    // and the five-block lanes are the low lane ids, so a CU's two workgroups -- ids c and c + 256 -- get nine between them).
    const bool wg_stats = a.part_rows != nullptr;
    const int stat_lanes = a.stat_lanes;
    if (wg_stats && lane_id >= stat_lanes) return;                      // the grid is rounded up to the XCD pattern (whole workgroups leave)
    const StatLane sl = wg_stats ? stat_lane_of(lane_id, stat_lanes, a.n_slots, a.Q, a.chunks) : StatLane{0, 0, 1};
    const int my_slot = sl.slot, slot_lanes = sl.L;
    const int part_idx = sl.slot + sl.j * a.n_slots;                    // where this lane's partial goes: slot = index % n_slots
    const int slot_items = wg_stats ? ((a.Q - my_slot + a.n_slots - 1) / a.n_slots) * a.chunks : 0;
    int run_n = 0;                                                      // rows merged so far (uniform)

    // ---- weight staging (transposing when the matrix is k-major) ----
    // shared weights: eight 16-byte loads in flight per thread before the first LDS write (unconditional, clamped addresses: a conditional
    // load sits in its own basic block and the 16 trips of the old loop were 16 dependent round trips at the head of every workgroup)
    auto put_weight = [&](int j, int k, const f32x4 &v) {
        if (BF) {
            if (X3) {
                bf16x4 b1, b2, b3;
                split3_bf16(v, b1, b2, b3);
                *reinterpret_cast<bf16x4 *>(sWb + j * LDB + k) = b1;
                *reinterpret_cast<bf16x4 *>(sWb + (CB + j) * LDB + k) = b2;
                *reinterpret_cast<bf16x4 *>(sWb + (2 * CB + j) * LDB + k) = b3;
            } else {
                bf16x4 b;
#pragma unroll
                for (int i = 0; i < 4; ++i) b[i] = (__bf16)v[i];
                *reinterpret_cast<bf16x4 *>(sWb + j * LDB + k) = b;
            }
        } else {
            *reinterpret_cast<f32x4 *>(sW + j * LDW + k) = v;
        }
    };
    auto stage_weights = [&](int pidx) {
        if (!perwin_w) {
            const float *Wg = a.W;
            constexpr int TOT = CB * (CIN / 4), SU = 8;
            const bool flip = POOL && a.pool_gamma != nullptr;
            for (int e0 = tid; e0 < TOT; e0 += PW_NW * 64 * SU) {
                f32x4 v[SU];
                float gs[SU];
#pragma unroll
                for (int u = 0; u < SU; ++u) {
                    const int e = e0 + u * PW_NW * 64;
                    const int j = (e < TOT ? e : 0) / (CIN / 4), k4 = e % (CIN / 4);
                    const int jj = cb0 + j < a.cout ? cb0 + j : 0;
                    v[u] = *reinterpret_cast<const f32x4 *>(Wg + (size_t)jj * a.ldw + 4 * k4);
                    gs[u] = flip ? a.pool_gamma[jj] : 1.f;
                }
#pragma unroll
                for (int u = 0; u < SU; ++u) {
                    const int e = e0 + u * PW_NW * 64;
                    if (e >= TOT) continue;
                    const int j = e / (CIN / 4), k4 = e % (CIN / 4);
                    f32x4 w = v[u];
                    if (cb0 + j >= a.cout) w = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (gs[u] < 0.f) w = -w;                                 // z' = sgn(gamma) z: the pool tracks max z'
                    put_weight(j, 4 * k4, w);
                }
            }
        } else {
            const float *Wg = a.W + (size_t)pidx * a.w_win_stride;   // [CIN][cout]
            for (int e = tid; e < CIN * CB; e += PW_NW * 64) {
                const int k = e / CB, j = e % CB;
                const float v = (cb0 + j < a.cout) ? Wg[(size_t)k * a.cout + cb0 + j] : 0.f;
                if (BF && X3) {
                    const __bf16 b1 = (__bf16)v;
                    const float r1 = v - (float)b1;
                    const __bf16 b2 = (__bf16)r1;
                    sWb[j * LDB + k] = b1;
                    sWb[(CB + j) * LDB + k] = b2;
                    sWb[(2 * CB + j) * LDB + k] = (__bf16)(r1 - (float)b2);
                } else if (BF) sWb[j * LDB + k] = (__bf16)v;
                else sW[j * LDW + k] = v;
            }
        }
    };

    // Consumer-side finalize of the INPUT's BatchNorm (kernels.h: PwGemm.pfin): the input BatchNorm's constants of this workgroup's slot from the
    // producer's per-workgroup partials in ONE memory round trip -- thread (gq, cq) takes the partials gq, gq + G, ... of the slot for the four
    // channels 4 cq .. 4 cq + 3 (16-byte loads, a batch of eight in flight).  The FIRST batch (all of them for <= 64 partials per slot) is
    // requested BEFORE the weight tile is staged, so that its round trip runs under the staging instead of after it (round 3 had it behind:
    // a dependent trip + the merge + two barriers in front of the first MFMA of every workgroup, +3 % on the pooled GEMM).
    constexpr int CQ = CIN / 4;                                    // channel quads
    constexpr int GW = 64 / CQ >= 1 ? 64 / CQ : 1;                 // groups per wave (2 at 128 channels, 4 at 64)
    constexpr int G = GW * PW_NW > 8 ? 8 : GW * PW_NW;             // groups in all
    constexpr int WV = G / GW;                                     // waves that take part
    static_assert(CQ <= 64 && G % GW == 0, "a wave holds whole groups");
    const bool pfin = PRO && a.pfin.part.sum != nullptr;
    const int cq = lane % CQ, gq = wave * GW + lane / CQ;
    const int per_slot_parts = pfin ? a.pfin.part.parts / a.n_slots : 0;
    f32x4 fv[8], fw[8];
    int frw[8];
    auto pfin_load = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int kk = k0 + G * u;
            const int idx = my_slot + (kk < per_slot_parts ? kk : 0) * a.n_slots;
            frw[u] = kk < per_slot_parts ? a.pfin.part.rows[idx] : 0;
            fv[u] = *reinterpret_cast<const f32x4 *>(a.pfin.part.sum + (size_t)idx * CIN + 4 * cq);
            fw[u] = *reinterpret_cast<const f32x4 *>(a.pfin.part.sq + (size_t)idx * CIN + 4 * cq);
        }
    };
    if (PRO) {
        if (pfin && gq < G && gq < per_slot_parts) pfin_load(gq);
    }
    if (!perwin_w) stage_weights(0);

    int staged_slot = -1;
    if (PRO && pfin) {
        // sums of n, n mean and M2 + n mean^2 in double, the groups of a wave are folded by shuffles and the waves through LDS in wave order:
        // fixed order, bitwise reproducible.  M2 = sum (M2_i + n_i mean_i^2) - N mean^2 in double is exact to ~1e-10 of M2 for fp32 partials
        // unless |mean| > 1e3 sigma.
        double *rsm = reinterpret_cast<double *>(sRed);                // [WV][CIN] sum n mean, then [WV][CIN] sum (M2 + n mean^2), [WV] n
        double *rsq = rsm + WV * CIN, *rnn = rsq + WV * CIN;
        double sn = 0.0, sm[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};
        if (gq < G) {
            for (int k0 = gq; k0 < per_slot_parts; k0 += G * 8) {
                if (k0 != gq) pfin_load(k0);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (frw[u] > 0) {
                        const double nn = (double)frw[u];
                        sn += nn;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const double m = (double)fv[u][i];
                            sm[i] += nn * m;
                            sq[i] += (double)fw[u][i] + nn * m * m;
                        }
                    }
                }
            }
        }
        // fold the groups of a wave (lanes cq, cq + CQ, ...), then the waves
#pragma unroll
        for (int off = CQ; off < 64; off <<= 1) {
            sn += __shfl_xor(sn, off);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sm[i] += __shfl_xor(sm[i], off);
                sq[i] += __shfl_xor(sq[i], off);
            }
        }
        if (wave < WV && lane < CQ) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                rsm[wave * CIN + 4 * cq + i] = sm[i];
                rsq[wave * CIN + 4 * cq + i] = sq[i];
            }
            if (lane == 0) rnn[wave] = sn;
        }
        __syncthreads();
        if (tid < CIN) {
            const int c = tid;
            double N = 0.0, S = 0.0, Q2 = 0.0;
#pragma unroll
            for (int w2 = 0; w2 < WV; ++w2) {
                N += rnn[w2];
                S += rsm[w2 * CIN + c];
                Q2 += rsq[w2 * CIN + c];
            }
            const double mean = N > 0.0 ? S / N : 0.0;
            double m2 = Q2 - N * mean * mean;
            if (m2 < 0.0) m2 = 0.0;
            const double var = N > 0.0 ? m2 / N : 0.0;              // bn_fwd_constants (bn_desc.h) is the definition of these lines
            const float invstd = (float)(1.0 / sqrt(var + (double)a.eps));
            const float sc = a.pfin.layer.gamma[c] * invstd;
            const float sh = a.pfin.layer.beta[c] - (float)mean * sc;
            sPro[c] = sc;
            sPro[CIN + c] = sh;
            if (sl.j == 0 && cb0 == 0) {                        // one writer per slot
                const size_t o = (size_t)my_slot * CIN + c;
                a.pfin.out.scale[o] = sc;
                a.pfin.out.shift[o] = sh;
                a.pfin.out.mean[o] = (float)mean;
                a.pfin.out.invstd[o] = invstd;
                a.pfin.out.smean[o] = (float)mean;
                a.pfin.out.suvar[o] = (float)(N > 1.0 ? m2 / (N - 1.0) : m2);
            }
        }
        staged_slot = my_slot;
        __syncthreads();                                        // sRed is free again, sPro is staged
    }
    const uint32_t dthr = drop_threshold(a.drop_p);
    const uint32_t dbase = a.drop_seed;
    const float dscale = PRO == 2 ? 1.0f / (1.0f - a.drop_p) : 1.0f;
    const bool do_stats = a.part_sum != nullptr;
    const bool do_store = a.Z != nullptr;

    float sgn[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = cb0 + 32 * t + r;
        sgn[t] = (POOL && a.pool_gamma && col < a.cout && a.pool_gamma[col] < 0.f) ? -1.0f : 1.0f;
    }
  const int it_end = wg_stats ? slot_items : n_rb, it_step = wg_stats ? slot_lanes : n_lanes;
  f32x4 xa[4][2];                     // split kernels: the A operand of four k steps (below); in flight ACROSS blocks of rows
  bool xa_primed = false;
  f32x2 s_sum2[NT], s_sq2[NT];
  float s_ext[NT], s_z0[NT], bias_v[NT], init_v[NT];
  int s_arg[NT];
  int s_cnt = 0;
  // Split kernels: a block of rows (a.chunk_rows of them, 128 from the host) belongs to ONE WAVE, which walks its tiles in row order:
  // the eight waves of the workgroup take blocks v, v + 8 L, ... (v = 8 j + wave) and never meet inside the loop -- no barrier per
  // block and no cross-wave merge of the pooled extremes (a wave writes its block's extremes itself); with a block shared by the
  // eight waves those two took a third of the kernel (in-kernel stamps, tools/x3_stamps.py).  The prologue constants of the
  // workgroup's one slot are staged before the loop.
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int it_first = X3 ? (wg_stats ? sl.j : lane_id) * PW_NW + wave_u : (wg_stats ? sl.j : lane_id);
  const int it_stride = X3 ? it_step * PW_NW : it_step;
  if (X3) {
      const int slot0 = wg_stats ? my_slot : 0;                   // eval mode has one slot
      if (PRO && slot0 != staged_slot) {
          for (int e = tid; e < CIN; e += PW_NW * 64) {
              sPro[e] = a.pro_scale[(size_t)slot0 * CIN + e];
              sPro[CIN + e] = a.pro_shift[(size_t)slot0 * CIN + e];
          }
          staged_slot = slot0;
      }
      __syncthreads();                                            // weights and constants are staged
  }
  // the sign that turns the tracked extreme of z' = sgn(gamma) z back into z, for the column this thread merges (one load, not one per block)
  const float sg_own = (POOL && a.pool_gamma && cb0 + tid < a.cout && tid < CB && a.pool_gamma[cb0 + tid] < 0.f) ? -1.0f : 1.0f;
  [[maybe_unused]] int stamp_n = 0;
  for (int it = it_first; it < it_end; it += it_stride) {
    const int q = wg_stats ? my_slot + (it / a.chunks) * a.n_slots : it / a.chunks;
    const int chunk = it % a.chunks;
    const int w_begin = a.uniform_rows > 0 ? q * a.uniform_rows : a.win_off[q];
    const int w_end = a.uniform_rows > 0 ? w_begin + a.uniform_rows : a.win_off[q + 1];
    const int row_begin = w_begin + chunk * a.chunk_rows;
    const int row_end = min(w_end, row_begin + a.chunk_rows);
    const int nrows = max(row_end - row_begin, 0);
    const int slot = (a.n_slots > 1) ? (q % a.n_slots) : 0;
    const int pidx = pidx_of(q, a.n_slots, a.Q, a.perwin_slot_major);

    // everything the previous block of rows read from LDS (prologue constants, per-window weights, reduction scratch) is done
    if (!X3) __syncthreads();
    const bool restage = !X3 && (perwin_w || (PRO && slot != staged_slot));
    if (restage) {
        if (perwin_w) stage_weights(pidx);
        if (PRO) {
            for (int e = tid; e < CIN; e += PW_NW * 64) {
                sPro[e] = a.pro_scale[(size_t)slot * CIN + e];
                sPro[CIN + e] = a.pro_shift[(size_t)slot * CIN + e];
            }
        }
        staged_slot = slot;
        __syncthreads();
    }

    // BatchNorm statistics are accumulated as sums of (v - z0) and (v - z0)^2 with z0 = the wave's first
    // row: E[z^2] - mean^2 in fp32 loses everything when a channel's spread is small against its mean
    // (the T-Net FC layers normalise over only B rows of near-identical pooled features).
    // MaxPool: BatchNorm + ReLU are monotone per channel with the direction of sign(gamma) (scale = gamma * invstd), so one
    // signed extreme per channel is enough: ext = max over rows of sgn * v (the sign is folded into the staged weights).
    // The accumulators start at bias - z0, so a finished tile holds d = z - z0 directly (no bias add, no subtraction per element:
    // VALU instructions do not overlap with fp32 MFMAs on this part -- tools/mfma_probe.hip -- so every epilogue instruction is
    // time taken from the matrix pipe).  z0 is only known after the wave's first tile of the block of rows: that tile starts at
    // bias and has z0 subtracted once it is known.
    // Per-WORKGROUP statistics (wg_stats: every train-mode point layer): the sums run over ALL blocks of rows the workgroup walks -- one
    // shift z0 per wave (its first row ever), one cross-wave merge after the last block -- instead of a merge per block.  Per block that
    // merge (a Chan step in double per wave and column by 128 threads, between two barriers) took 39 % of the split pooled kernel
    // (in-kernel stamps, tools/x3_stamps.py) and was the round-3 regression of the fp32 one (the running merge into sRun came with the
    // per-workgroup partials).  Per block only the pooled layers still combine their extremes across the waves.
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = cb0 + 32 * t + r;
        if (!wg_stats || it == it_first) {
            s_z0[t] = 0.f;
            s_sum2[t] = f32x2{0.f, 0.f};
            s_sq2[t] = f32x2{0.f, 0.f};
        }
        bias_v[t] = (!X3 && a.bias && col < a.cout) ? sgn[t] * a.bias[(size_t)(a.bias_win_stride ? pidx : 0) * a.bias_win_stride + col] : 0.f;
        // T-Net fc_3: the k x k output has the identity added (pointnetAtt.py:42-46): +1 on the columns i * (k + 1) of the k * k
        if (!X3 && a.identity_k > 0 && col < a.cout && col % (a.identity_k + 1) == 0) bias_v[t] += 1.0f;
        s_ext[t] = -__builtin_inff();
        s_arg[t] = -1;
    }
    if (!wg_stats || it == it_first) s_cnt = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) init_v[t] = bias_v[t] - s_z0[t];           // (z0 = 0 until the wave's first tile has set it)

    // The epilogue of one finished 32-row tile (accumulators `acc`, rows row0 .. row0 + valid - 1).  first: the wave's first tile of this block
    // of rows (its row 0 becomes the shift z0 of the statistics); fresh: the accumulators started at the bias (z0 was not known yet).
    auto finish_tile = [&](f32x16 (&acc)[NT], const int row0, const int valid, const bool first, const bool fresh) {
        // ---- epilogue: lane = output channel, registers = 16 rows; predicated, no branch between elements ----
        if (do_stats) {
            if (first) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float z0 = __shfl(acc[t][0], r);            // row0 + 0 lives in lane r, register 0 (bias included)
                    s_z0[t] = z0;
                    init_v[t] = bias_v[t] - z0;
                }
            }
            if (fresh) {                                   // this tile's accumulators started at the bias, not at bias - z0
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[t][e] -= s_z0[t];
            }
            s_cnt += valid;
        }
        // FULL: all 32 rows of the tile exist (every tile but a window's last): no row predicate at all.  STATS is a compile-time
        // copy of do_stats: as a run-time flag the compiler turned every `s_sum += d` into an add AND a select
        auto epilogue = [&](auto full_tag, auto stats_tag) {
            constexpr bool FULL = decltype(full_tag)::value;
            constexpr bool STATS = decltype(stats_tag)::value;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int col = cb0 + 32 * t + r;
                // split kernels: whole column blocks only and the store decided at compile time (the pooled layers never store) -- as run-time
                // lane conditions these are an exec-mask branch around every pair of elements, stores or not
                const bool cok = X3 || col < a.cout;
                const float z0 = STATS ? s_z0[t] : 0.f;
                // pooled layers track z' = sgn(gamma) z (signed weights): the stored Z is z, so the sign comes back off (exact)
                const float zs = POOL ? sgn[t] : 1.0f;
                float *zp = a.Z + (size_t)row0 * a.ldz + col;
#pragma unroll
                for (int e = 0; e < 16; e += 2) {
                    const int rr0 = (e & 3) + 8 * (e >> 2) + 4 * h;       // e even: rows rr0 and rr0 + 1
                    const bool ok0 = FULL || rr0 < valid, ok1 = FULL || rr0 + 1 < valid;
                    const float d0 = acc[t][e], d1 = acc[t][e + 1];
                    if ((X3 ? !POOL : do_store) && cok) {
                        if (BF && ZBF) {
                            if (ok0) reinterpret_cast<__bf16 *>(a.Z)[((size_t)row0 + rr0) * a.ldz + col] = (__bf16)(zs * (d0 + z0));
                            if (ok1) reinterpret_cast<__bf16 *>(a.Z)[((size_t)row0 + rr0 + 1) * a.ldz + col] = (__bf16)(zs * (d1 + z0));
                        } else {
                            if (STREAM) {
                                if (ok0) st_stream(zs * (d0 + z0), &zp[(size_t)rr0 * a.ldz]);
                                if (ok1) st_stream(zs * (d1 + z0), &zp[(size_t)(rr0 + 1) * a.ldz]);
                            } else {
                                if (ok0) zp[(size_t)rr0 * a.ldz] = zs * (d0 + z0);
                                if (ok1) zp[(size_t)(rr0 + 1) * a.ldz] = zs * (d1 + z0);
                            }
                        }
                    }
                    if (STATS) {
                        const f32x2 d2 = {ok0 ? d0 : 0.f, ok1 ? d1 : 0.f};
                        s_sum2[t] += d2;
                        s_sq2[t] = __builtin_elementwise_fma(d2, d2, s_sq2[t]);
                    }
                    if (POOL) {
                        // d is sgn(gamma) * z - z0 (signed weights): same order as z; strict compare: rows ascend, the first extreme wins
                        const float v0 = ok0 ? d0 : -__builtin_inff(), v1 = ok1 ? d1 : -__builtin_inff();
                        if constexpr (ARG) {
                            const bool g0 = v0 > s_ext[t];
                            s_ext[t] = g0 ? v0 : s_ext[t];
                            s_arg[t] = g0 ? row0 + rr0 : s_arg[t];
                            const bool g1 = v1 > s_ext[t];
                            s_ext[t] = g1 ? v1 : s_ext[t];
                            s_arg[t] = g1 ? row0 + rr0 + 1 : s_arg[t];
                        } else {
                            s_ext[t] = fmaxf(s_ext[t], fmaxf(v0, v1));              // one v_max3_f32
                        }
                    }
                }
            }
        };
        if (do_stats) {
            if (valid == 32) epilogue(std::true_type{}, std::true_type{});
            else epilogue(std::false_type{}, std::true_type{});
        } else {
            if (valid == 32) epilogue(std::true_type{}, std::false_type{});
            else epilogue(std::false_type{}, std::false_type{});
        }
    };

    if constexpr (X3) {
        // ---- split kernels: ONE wave per SIMD with the whole register file (512 per lane) and 64 rows per wave: two 32-row sub-tiles share
        // every weight fragment read from LDS, and there is room to keep a k step's operands ahead of its MFMAs ----
        static_assert(PRO != 2 && NBLK >= 1, "the split kernels have no dropout prologue");
        constexpr int RT = XRT;
        const int nst = (nrows + 31) / 32;                   // 32-row sub-tiles of this block of rows
        // Two waves per SIMD (8-wave workgroup, one per CU): a wave's step is a VALU phase (BatchNorm + ReLU, the three-term split: ~50
        // instructions) and an MFMA phase (6 * NT = 24 MFMAs, 768 cycles of the SIMD's matrix pipe); the partner wave fills the pipe during the
        // VALU phase and the epilogue.  The A operand of a k step (16 k of 32 rows: two 16-byte loads per lane) is requested THREE steps ahead
        // into one of four register buffers addressed by step parity mod 4 (8 steps per tile: a tile starts at buffer 0 again, no copies):
        // with one 32-k block ahead (two steps) the waves spent 30 % of their time in s_waitcnt vmcnt (rocprofv3 SQ_WAIT_INST_ANY).
        static_assert(RT == 1 && (2 * NBLK) % 4 == 0, "step parity addresses the four A buffers");
        constexpr int NSTEP = 2 * NBLK, AHEAD = 3;
        auto load_step = [&](f32x4 (&dst)[2], int rb_, int re_, int st_, int step_) {
            // rows past the block's end re-read its last row: their products are never used
            const int row = min(rb_ + st_ * 32 + r, re_ - 1);
            const float *ap = a.A + (size_t)row * a.lda + 16 * step_ + 8 * h;
            if (STREAM_LD) {
                dst[0] = ld_stream(reinterpret_cast<const f32x4 *>(ap));
                dst[1] = ld_stream(reinterpret_cast<const f32x4 *>(ap + 4));
            } else {
                dst[0] = *reinterpret_cast<const f32x4 *>(ap);
                dst[1] = *reinterpret_cast<const f32x4 *>(ap + 4);
            }
        };
        // the wave's first tile of the NEXT block of rows this workgroup walks: its first steps are requested under the last tile of this
        // block, so the pipeline does not drain at the block boundary (reduction + barriers run over loads in flight)
        int rb_n = row_begin, re_n = row_end;
        bool next_ok = false;
        if (it + it_stride < it_end) {
            const int it_n = it + it_stride;
            const int q_n = wg_stats ? my_slot + (it_n / a.chunks) * a.n_slots : it_n / a.chunks;
            const int wb_n = a.uniform_rows > 0 ? q_n * a.uniform_rows : a.win_off[q_n];
            const int we_n = a.uniform_rows > 0 ? wb_n + a.uniform_rows : a.win_off[q_n + 1];
            const int b_n = wb_n + (it_n % a.chunks) * a.chunk_rows, e_n = min(we_n, b_n + a.chunk_rows);
            if (e_n > b_n) {
                next_ok = true;
                rb_n = b_n;
                re_n = e_n;
            }
        }
        PW_STAMP(1);                                         // block of rows begins (after the barrier)
        int st0 = 0;
        if (st0 < nst && !xa_primed) {
#pragma unroll
            for (int p = 0; p < AHEAD; ++p) load_step(xa[p], row_begin, row_end, st0, p);
        }
        for (; st0 < nst; ++st0) {
            const bool fresh0 = s_cnt == 0;                  // the wave's first tile ever: its row 0 is the shift of the statistics
            const bool more = st0 + 1 < nst;
            // where the tail of this tile prefetches: the block's next tile, the first tile of the wave's next block, or (nothing left) itself
            const int p_rb = more ? row_begin : rb_n, p_re = more ? row_end : re_n;
            const int p_st = more ? st0 + 1 : (next_ok ? 0 : st0);
            f32x16 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[t][e] = init_v[t];
            PW_STAMP(2);                                     // tile begins
            int wb01 = r * LDB + 8 * h, wb2 = wb01 + 2 * CB * LDB;       // element offsets into sWb (the pointer itself keeps its LDS address space)
            asm volatile("" : "+v"(wb01), "+v"(wb2));                    // opaque per tile: nothing to hoist out of the loops
#pragma unroll
            for (int sp = 0; sp < NSTEP; ++sp) {
                // request step sp + AHEAD (unconditional: behind a branch the wait counts below turn conservative, vmcnt(0) at the tile's end)
                if (sp + AHEAD < NSTEP) load_step(xa[(sp + AHEAD) & 3], row_begin, row_end, st0, sp + AHEAD);
                else load_step(xa[(sp + AHEAD) & 3], p_rb, p_re, p_st, sp + AHEAD - NSTEP);
                __builtin_amdgcn_sched_barrier(0);       // the prefetch stays HERE (in the unrolled body the scheduler sinks loads to their use)
                const int k0 = 16 * sp + 8 * h;
                f32x4 lo = xa[sp & 3][0], hi = xa[sp & 3][1];
                if (PRO) {
                    const f32x4 sc0 = *reinterpret_cast<const f32x4 *>(sPro + k0), sc1 = *reinterpret_cast<const f32x4 *>(sPro + k0 + 4);
                    const f32x4 sh0 = *reinterpret_cast<const f32x4 *>(sPro + CIN + k0), sh1 = *reinterpret_cast<const f32x4 *>(sPro + CIN + k0 + 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        lo[i] = fmaxf(fmaf(lo[i], sc0[i], sh0[i]), 0.f);
                        hi[i] = fmaxf(fmaf(hi[i], sc1[i], sh1[i]), 0.f);
                    }
                }
                bf16x8 a1, a2, a3, b1[NT], b2[NT], b3[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    // two lane bases + immediates (the three images span 104 KB, a ds_read offset reaches 64 KB): left to itself the compiler kept
                    // sixteen address registers for these reads in the kernel that also stores Z, spilled them, and every reload in the k loop
                    // waited for ALL global loads in flight (scratch reloads count on vmcnt)
                    b1[t] = *reinterpret_cast<const bf16x8 *>(sWb + wb01 + (32 * t) * LDB + 16 * sp);
                    b2[t] = *reinterpret_cast<const bf16x8 *>(sWb + wb01 + (CB + 32 * t) * LDB + 16 * sp);
                    b3[t] = *reinterpret_cast<const bf16x8 *>(sWb + wb2 + (32 * t) * LDB + 16 * sp);
                }
                split3_bf16(lo, hi, a1, a2, a3);
                // six exact partial products per tile; one accumulator takes its six back to back (a dependent chain of this MFMA issues at
                // full rate)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1[t], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3[t], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2[t], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b1[t], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2[t], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1[t], acc[t], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);   // steps do not mix: the unrolled body would otherwise hoist reads for several steps and spill
            }
            PW_STAMP(3);                                     // k loop issued
            const int row0 = row_begin + st0 * 32;
            finish_tile(acc, row0, min(32, row_end - row0), fresh0, fresh0);
            PW_STAMP(4);                                     // epilogue done
        }
        xa_primed = nst > 0 && next_ok;
    } else {
    const int ntiles = (nrows + 31) / 32;
    // A fragments: blocks of 4 j (= 32 k = one 128-byte line per row), the next block prefetched in registers
    // while the current one feeds 16 * NT MFMAs.  The prefetch runs across tile boundaries.
    f32x4 a_cur[4], a_nxt[4], a_nx2[4];
    // bf16 kernels: the matrix work of a 32-k block is 8 MFMAs of 32 cycles, far shorter than a trip to HBM, so ONE block in flight per
    // wave caps the kernel at bytes-in-flight / latency (about 4 TB/s measured); they keep TWO blocks in flight (a_nxt, a_nx2)
    // (fp32 kernels with NT <= 2 -- <= 1 us of matrix work per block and wave, 4.4 .. 4.8 TB/s -- were tried with two blocks in flight as well in
    // round 3: every one of them 1 .. 13 % SLOWER on the same box (gpurun_out r3C): they do not wait for their loads either.)
    constexpr int PF = BF ? 2 : 1;

    auto frag_ptr = [&](int tile, int kb) -> const float * {
        const int row0 = row_begin + tile * 32;
        const int valid = min(32, row_end - row0);
        const int arow = row0 + min(r, valid - 1);
        return a.A + (size_t)arow * a.lda + 32 * kb + (BF ? 8 : 4) * h;
    };
    // float offset of the j-th 16-byte piece of a 32-k block: fp32 k = 8 j + 4 h .. + 3; bf16 k = 16 (j / 2) + 8 h + 4 (j & 1) .. + 3
    auto frag_off = [](int j) -> int { return BF ? 16 * (j >> 1) + 4 * (j & 1) : 8 * j; };

    // A stored as bf16 (ampnet precision mode 3, BF kernels only): the 8 consecutive k of an MFMA step are ONE 16-byte load; the raw
    // bits ride in a_cur[2 s] / a_nxt[2 s] (the odd entries stay unused) and are widened to fp32 for the prologue
    constexpr bool a_bf = BF && ABF;
    auto load_frags = [&](f32x4 (&dst)[4], int t_, int kb_) {
        if (a_bf) {
            const int row0_ = row_begin + t_ * 32;
            const int arow_ = row0_ + min(r, min(32, row_end - row0_) - 1);
            const __bf16 *ap = reinterpret_cast<const __bf16 *>(a.A) + (size_t)arow_ * a.lda + 32 * kb_ + 8 * h;
            dst[0] = *reinterpret_cast<const f32x4 *>(ap);
            dst[2] = *reinterpret_cast<const f32x4 *>(ap + 16);
        } else {
            const float *ap = frag_ptr(t_, kb_);
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[j] = STREAM_LD ? ld_stream(reinterpret_cast<const f32x4 *>(ap + frag_off(j))) : *reinterpret_cast<const f32x4 *>(ap + frag_off(j));
        }
    };
    int tile = wave;
    if (tile < ntiles) load_frags(a_cur, tile, 0);
    if (PF == 2) {                                        // prime the second stage: block 1 of this tile, or block 0 of the wave's next tile
        int ptile = tile, pkb = 1;
        if (pkb >= NBLK) {
            ptile += PW_NW;
            pkb = 0;
        }
        if (ptile < ntiles) load_frags(a_nxt, ptile, pkb);
    }
    auto pro_apply = [&](f32x4 v, const f32x4 &sc, const f32x4 &sh, int row, int k0) -> f32x4 {
        if (PRO) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaxf(fmaf(v[i], sc[i], sh[i]), 0.f);
            if (PRO == 2) {
                const uint32_t e0 = (uint32_t)row * (uint32_t)CIN + (uint32_t)k0;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = (mix32((e0 + i) ^ dbase) >= dthr) ? v[i] * dscale : 0.f;
            }
        }
        return v;
    };
    auto arow_of = [&](int t_) -> int {
        const int row0_ = row_begin + t_ * 32;
        return row0_ + min(r, min(32, row_end - row0_) - 1);
    };
    f32x4 pbv[NT], pav = {0.f, 0.f, 0.f, 0.f};            // PIPE: operands of the step about to run
    if (PIPE && !BF && tile < ntiles) {
        const int k0 = 4 * h;
#pragma unroll
        for (int t = 0; t < NT; ++t) pbv[t] = *reinterpret_cast<const f32x4 *>(sW + (32 * t + r) * LDW + k0);
        f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
        if (PRO) {
            sc = *reinterpret_cast<const f32x4 *>(sPro + k0);
            sh = *reinterpret_cast<const f32x4 *>(sPro + CIN + k0);
        }
        pav = pro_apply(a_cur[0], sc, sh, arow_of(tile), k0);
    }
    for (; tile < ntiles; tile += PW_NW) {
        const int row0 = row_begin + tile * 32;
        const int valid = min(32, row_end - row0);
        const int arow = row0 + min(r, valid - 1);
        const int arow_next = (tile + PW_NW < ntiles) ? arow_of(tile + PW_NW) : arow;
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][e] = init_v[t];

        // the pipelined fp32 loop is unrolled over its k blocks: the LDS offsets of the operand reads become immediates
        // (25 integer VALU instructions per block of 64 MFMAs otherwise -- and VALU time is matrix-pipe time here)
        constexpr int KB_UNROLL = (PIPE && !BF && CIN <= 128) ? NBLK : 1;
#pragma unroll KB_UNROLL
        for (int kb = 0; kb < NBLK; ++kb) {
            // prefetch the next block (same tile, or block 0 of this wave's next tile)
            {
                int ptile = tile, pkb = kb + PF;
                while (pkb >= NBLK) {
                    ptile += PW_NW;
                    pkb -= NBLK;
                }
                if (ptile < ntiles) load_frags(PF == 2 ? a_nx2 : a_nxt, ptile, pkb);
            }
            if (BF) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const int k0 = 32 * kb + 16 * s2 + 8 * h;
                    f32x4 lo = a_cur[2 * s2], hi = a_cur[2 * s2 + 1];
                    if (a_bf) {
                        const bf16x8 raw = __builtin_bit_cast(bf16x8, a_cur[2 * s2]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            lo[i] = (float)raw[i];
                            hi[i] = (float)raw[4 + i];
                        }
                    }
                    if (PRO) {
                        const f32x4 sc0 = *reinterpret_cast<const f32x4 *>(sPro + k0), sc1 = *reinterpret_cast<const f32x4 *>(sPro + k0 + 4);
                        const f32x4 sh0 = *reinterpret_cast<const f32x4 *>(sPro + CIN + k0), sh1 = *reinterpret_cast<const f32x4 *>(sPro + CIN + k0 + 4);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            lo[i] = fmaxf(fmaf(lo[i], sc0[i], sh0[i]), 0.f);
                            hi[i] = fmaxf(fmaf(hi[i], sc1[i], sh1[i]), 0.f);
                        }
                        if (PRO == 2) {
                            const uint32_t e0 = (uint32_t)arow * (uint32_t)CIN + (uint32_t)k0;
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                lo[i] = (mix32((e0 + i) ^ dbase) >= dthr) ? lo[i] * dscale : 0.f;
                                hi[i] = (mix32((e0 + 4 + i) ^ dbase) >= dthr) ? hi[i] * dscale : 0.f;
                            }
                        }
                    }
                    const bf16x8 av = pack_bf16(lo, hi);
                    bf16x8 bw[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) bw[t] = *reinterpret_cast<const bf16x8 *>(sWb + (32 * t + r) * LDB + k0);
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bw[t], acc[t], 0, 0, 0);
                }
            }
            if (PIPE && !BF) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // the step after this one: (kb, j + 1), or step 0 of the next k block / of this wave's next tile
                    const bool wrap = j == 3;
                    const int k0n = (wrap ? (32 * (kb + 1)) % CIN : 32 * kb + 8 * (j + 1)) + 4 * h;
                    const int row_n = (wrap && kb == NBLK - 1) ? arow_next : arow;
                    f32x4 sc_n = {1.f, 1.f, 1.f, 1.f}, sh_n = {0.f, 0.f, 0.f, 0.f}, av_n = pav;
                    if constexpr (NT == 4) {
                        // two groups of two column tiles, the MFMAs of a group alternate accumulators; a group's weights are dead once its
                        // eight MFMAs are issued and are re-fetched for the next step in the shadow of the other group
#pragma unroll
                        for (int gq = 0; gq < 2; ++gq) {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
#pragma unroll
                                for (int t = 2 * gq; t < 2 * gq + 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(pav[i], pbv[t][i], acc[t], 0, 0, 0);
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int t = 2 * gq; t < 2 * gq + 2; ++t) pbv[t] = *reinterpret_cast<const f32x4 *>(sW + (32 * t + r) * LDW + k0n);
                            if (PRO && gq == 0) {
                                sc_n = *reinterpret_cast<const f32x4 *>(sPro + k0n);
                                sh_n = *reinterpret_cast<const f32x4 *>(sPro + CIN + k0n);
                            }
                            if (gq == 1) av_n = pro_apply(wrap ? a_nxt[0] : a_cur[(j + 1) & 3], sc_n, sh_n, row_n, k0n);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    } else {
                        f32x4 bn[NT];
#pragma unroll
                        for (int t = 0; t < NT; ++t) bn[t] = *reinterpret_cast<const f32x4 *>(sW + (32 * t + r) * LDW + k0n);
                        if (PRO) {
                            sc_n = *reinterpret_cast<const f32x4 *>(sPro + k0n);
                            sh_n = *reinterpret_cast<const f32x4 *>(sPro + CIN + k0n);
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(pav[i], pbv[t][i], acc[t], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        av_n = pro_apply(wrap ? a_nxt[0] : a_cur[(j + 1) & 3], sc_n, sh_n, row_n, k0n);
#pragma unroll
                        for (int t = 0; t < NT; ++t) pbv[t] = bn[t];
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    pav = av_n;
                }
            }
#pragma unroll
            for (int j = 0; j < ((BF || PIPE) ? 0 : 4); ++j) {
                const int k0 = 32 * kb + 8 * j + 4 * h;
                f32x4 av = a_cur[j];
                if (PRO) {
                    const f32x4 sc = *reinterpret_cast<const f32x4 *>(sPro + k0);
                    const f32x4 sh = *reinterpret_cast<const f32x4 *>(sPro + CIN + k0);
#pragma unroll
                    for (int i = 0; i < 4; ++i) av[i] = fmaxf(fmaf(av[i], sc[i], sh[i]), 0.f);
                    if (PRO == 2) {
                        const uint32_t e0 = (uint32_t)arow * (uint32_t)CIN + (uint32_t)k0;
#pragma unroll
                        for (int i = 0; i < 4; ++i) av[i] = (mix32((e0 + i) ^ dbase) >= dthr) ? av[i] * dscale : 0.f;
                    }
                }
                f32x4 bv[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const f32x4 *>(sW + (32 * t + r) * LDW + k0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[t][i], acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a_cur[j] = a_nxt[j];
                if (PF == 2) a_nxt[j] = a_nx2[j];
            }
        }

        {
            const bool first_tile = wg_stats ? s_cnt == 0 : tile == wave;     // whose row 0 becomes the statistics' shift
            finish_tile(acc, row0, valid, first_tile, first_tile);
        }
    }
    }

    const bool blk_stats = !wg_stats && do_stats;       // per-workgroup statistics are merged once, after the last block
    if (!blk_stats && !POOL) continue;
    if constexpr (X3 && POOL) {
        // the block was this wave's alone: combine the two half-waves and write its extremes (empty block: -inf / -1, as pool_finalize expects)
        const size_t o0 = (size_t)(q * a.chunks + chunk) * a.cout + cb0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float o_ext = __shfl_xor(s_ext[t], 32);
            const int o_arg = __shfl_xor(s_arg[t], 32);
            float f_ext = s_ext[t];
            int f_arg = s_arg[t];
            if (o_ext > f_ext || (o_ext == f_ext && (unsigned)o_arg < (unsigned)f_arg)) {
                f_ext = o_ext;
                f_arg = o_arg;
            }
            if (h == 0) {
                a.part_max[o0 + 32 * t + r] = (f_ext + s_z0[t]) * sgn[t];        // back from d = z' - z0 to z
                if (ARG) a.part_amax[o0 + 32 * t + r] = f_arg;
            }
        }
        continue;
    }

    // ---- combine the two half-waves, then the waves ----
    float *red_f = sRed;                                           // [PW_NW][CB][4]: S1, S2, ext, z0
    int *red_i = reinterpret_cast<int *>(sRed + PW_NW * CB * 4);   // [PW_NW][CB]: arg
    int *red_n = red_i + PW_NW * CB;                               // [PW_NW] rows seen by the wave
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float m_sum = s_sum2[t][0] + s_sum2[t][1], m_sq = s_sq2[t][0] + s_sq2[t][1];
        const float o_sum = __shfl_xor(m_sum, 32), o_sq = __shfl_xor(m_sq, 32);
        const float o_ext = __shfl_xor(s_ext[t], 32);
        const int o_arg = __shfl_xor(s_arg[t], 32);
        float f_ext = s_ext[t];
        int f_arg = s_arg[t];
        if (o_ext > f_ext || (o_ext == f_ext && (unsigned)o_arg < (unsigned)f_arg)) {
            f_ext = o_ext;
            f_arg = o_arg;
        }
        if (h == 0) {
            const int c = 32 * t + r;
            red_f[(wave * CB + c) * 4 + 0] = m_sum + o_sum;
            red_f[(wave * CB + c) * 4 + 1] = m_sq + o_sq;
            red_f[(wave * CB + c) * 4 + 2] = f_ext + s_z0[t];     // back from d = z - z0 (the waves have different z0)
            red_f[(wave * CB + c) * 4 + 3] = s_z0[t];
            red_i[wave * CB + c] = f_arg;
        }
    }
    if (lane == 0) red_n[wave] = s_cnt;
    PW_STAMP(6);                                             // partials written
    __syncthreads();
    PW_STAMP(7);                                             // all waves arrived
    for (int c = tid; c < CB; c += PW_NW * 64) {
        const int col = cb0 + c;
        if (col >= a.cout) continue;
        double n = 0.0, mean = 0.0, m2 = 0.0;                      // Chan's pairwise merge, fixed wave order
        float ext = -__builtin_inff();
        int arg = -1;
#pragma unroll
        for (int w = 0; w < PW_NW; ++w) {
            const double nw = (double)red_n[w];
            if (blk_stats && nw > 0.0) {
                // reciprocals of the (small integer) row counts by v_rcp_f64 + two Newton steps instead of four IEEE divisions per
                // wave: this merge sits between two barriers, i.e. on every wave's critical path (28 % of a bf16 block of rows)
                const double s1 = red_f[(w * CB + c) * 4 + 0], s2 = red_f[(w * CB + c) * 4 + 1];
                const double nn = n + nw;
                const double inv_nw = rcp_f64(nw), inv_nn = rcp_f64(nn);
                const double mw = (double)red_f[(w * CB + c) * 4 + 3] + s1 * inv_nw;
                const double m2w = s2 - s1 * s1 * inv_nw;
                const double delta = mw - mean, wgt = nw * inv_nn;
                mean += delta * wgt;
                m2 += m2w + delta * delta * n * wgt;
                n = nn;
            }
            const float ve = red_f[(w * CB + c) * 4 + 2];
            const int ie = red_i[w * CB + c];
            if (ve > ext || (ve == ext && (unsigned)ie < (unsigned)arg)) {
                ext = ve;
                arg = ie;
            }
        }
        const size_t o = (size_t)(q * a.chunks + chunk) * a.cout + col;
        const float sg = sg_own;
        if (blk_stats) {
            a.part_sum[o] = sg * (float)mean;       // chunk mean (of z, not of the signed z')
            a.part_sq[o] = (float)(m2 < 0.0 ? 0.0 : m2);   // chunk sum of squared deviations
        }
        if (POOL) {
            a.part_max[o] = ext * sg;               // the extreme itself (max for gamma >= 0, min otherwise)
            if (ARG) a.part_amax[o] = arg;
        }
    }
    run_n += nrows;
    PW_STAMP(5);                                             // block's reduction done
  }   // blocks of rows
#ifdef AMPNET_PW_STAMPS
    if (X3 && blockIdx.x == 0 && threadIdx.x == 0) g_pw_stamps[0] = (unsigned long long)stamp_n;
#endif
    if (!(wg_stats && do_stats)) return;
    {
        // the one cross-wave merge: per wave (rows, S1, S2, z0) over every block it walked -> Chan, fixed wave order
        float *red_f = sRed;
        int *red_n = reinterpret_cast<int *>(sRed + PW_NW * CB * 4) + PW_NW * CB;
        __syncthreads();                                        // the last block's pool merge has read the scratch
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float m_sum = s_sum2[t][0] + s_sum2[t][1], m_sq = s_sq2[t][0] + s_sq2[t][1];
            const float o_sum = __shfl_xor(m_sum, 32), o_sq = __shfl_xor(m_sq, 32);
            if (h == 0) {
                const int c = 32 * t + r;
                red_f[(wave * CB + c) * 4 + 0] = m_sum + o_sum;
                red_f[(wave * CB + c) * 4 + 1] = m_sq + o_sq;
                red_f[(wave * CB + c) * 4 + 3] = s_z0[t];
            }
        }
        if (lane == 0) red_n[wave] = s_cnt;
        __syncthreads();
        if (tid < CB) {
            const int c = tid;
            double n = 0.0, mean = 0.0, m2 = 0.0;
            int rows = 0;
#pragma unroll
            for (int w = 0; w < PW_NW; ++w) {
                const double nw = (double)red_n[w];
                rows += red_n[w];
                if (nw > 0.0) {
                    const double s1 = red_f[(w * CB + c) * 4 + 0], s2 = red_f[(w * CB + c) * 4 + 1];
                    const double nn = n + nw;
                    const double inv_nw = rcp_f64(nw), inv_nn = rcp_f64(nn);
                    const double mw = (double)red_f[(w * CB + c) * 4 + 3] + s1 * inv_nw;
                    const double m2w = s2 - s1 * s1 * inv_nw;
                    const double delta = mw - mean, wgt = nw * inv_nn;
                    mean += delta * wgt;
                    m2 += m2w + delta * delta * n * wgt;
                    n = nn;
                }
            }
            sRun[2 * c] = mean;
            sRun[2 * c + 1] = m2 < 0.0 ? 0.0 : m2;
            run_n = rows;
        } else {
            int rows = 0;
#pragma unroll
            for (int w = 0; w < PW_NW; ++w) rows += red_n[w];
            run_n = rows;
        }
    }
    // ---- the workgroup's partial (thread c wrote sRun[c] itself: no barrier needed), or the finished BatchNorm constants ----
    for (int c = tid; c < CB; c += PW_NW * 64) {
        const int col = cb0 + c;
        if (col >= a.cout) continue;
        const double mean = run_n > 0 ? sRun[2 * c] : 0.0, m2 = run_n > 0 ? sRun[2 * c + 1] : 0.0;
        if (a.fin.out.scale) {                          // one lane per slot: this workgroup saw every row of its slot
            const double N = (double)run_n;
            const double var = N > 0.0 ? m2 / N : 0.0;          // bn_fwd_constants / bn_fwd_store (bn_desc.h) are the definition of these lines
            const float invstd = (float)(1.0 / sqrt(var + (double)a.eps));
            const size_t o = (size_t)my_slot * a.cout + col;
            const float sc = a.fin.layer.gamma[col] * invstd;
            a.fin.out.scale[o] = sc;
            a.fin.out.shift[o] = a.fin.layer.beta[col] - (float)mean * sc;
            if (a.fin.out.mean) a.fin.out.mean[o] = (float)mean;
            if (a.fin.out.invstd) a.fin.out.invstd[o] = invstd;
            if (a.fin.out.smean) {
                a.fin.out.smean[o] = (float)mean;
                a.fin.out.suvar[o] = (float)(N > 1.0 ? m2 / (N - 1.0) : m2);
            }
        } else {
            // pooled layers: the statistics were taken of z' = sgn(gamma) z -- the mean changes sign back, M2 does not care
            const float sg = (POOL && a.pool_gamma && a.pool_gamma[col] < 0.f) ? -1.0f : 1.0f;
            a.part_sum[(size_t)part_idx * a.cout + col] = sg * (float)mean;
            a.part_sq[(size_t)part_idx * a.cout + col] = (float)m2;
        }
    }
    if (tid == 0 && cb0 == 0 && !a.fin.out.scale) {
        a.part_rows[part_idx] = run_n;
        // slots with one lane fewer than the widest leave their last partial slot empty: mark it (rows 0) for bn_finalize
        if (sl.j == sl.L - 1 && sl.L < (stat_lanes + a.n_slots - 1) / a.n_slots) a.part_rows[part_idx + a.n_slots] = 0;
    }
}

template <int CIN, int NT, int PRO, bool POOL, bool BF, bool ABF = false, bool ZBF = false, bool PIPE = false, bool ARG = true, bool X3 = false, int NW = PW_NW, int XRT = 1>
static int launch_pw_y(const PwGemm &a, hipStream_t st)
{
    constexpr int CB = 32 * NT;
    constexpr size_t lds_main = BF ? (size_t)(X3 ? 3 : 1) * CB * (CIN + 8) * 2 + (size_t)2 * CIN * sizeof(float) : (size_t)(CB * (CIN + 4) + 2 * CIN) * sizeof(float);
    constexpr size_t lds_red0 = (size_t)(NW * CB * 5 + NW) * sizeof(float) + (size_t)CB * 2 * sizeof(double);   // + sRun
    constexpr size_t lds_pfin = (size_t)(4 * 2 * CIN + 8) * sizeof(double);                   // scratch of the consumer-side BatchNorm finalize (same region)
    constexpr size_t lds_red = lds_red0 > lds_pfin ? lds_red0 : lds_pfin;
    constexpr size_t lds = lds_main + lds_red;
    static_assert(lds <= 160 * 1024, "LDS budget of a CU");
    static int resident = 0;           // workgroups the device holds at once (CUs x occupancy), measured once per instantiation
    constexpr auto kern = pw_gemm_kernel<CIN, NT, PRO, POOL, BF, ABF, ZBF, PIPE, ARG, X3, NW, XRT>;
    if (resident == 0) {
        if (lds > 65536) {
            if (int rc = allow_dynamic_lds<kern>(lds, "pw_gemm")) return rc;
        }
        int per_cu = 0, dev = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(kern), NW * 64, lds) != hipSuccess || per_cu < 1) per_cu = 1;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        resident = per_cu * cus;
    }
    // persistent grid: as many workgroups as fit at once, in units of (8 XCDs x column blocks); never more lanes than blocks of rows
    const int n_rb = a.Q * a.chunks, ncb = cdiv(a.cout, CB);
    int lanes = (resident / (8 * ncb)) * 8;
    if (lanes < 8) lanes = 8;
    if (lanes > cdiv(n_rb, 8) * 8) lanes = cdiv(n_rb, 8) * 8;
    if (a.part_rows) lanes = cdiv(a.stat_lanes, 8) * 8;                // per-workgroup statistics: the plan fixes the lanes (pw_gemm_stat_plan)
    dim3 grid((unsigned)(lanes * ncb));
    char name[64];
    snprintf(name, sizeof(name), "pw_gemm<%d,%d>%s%s%s", CIN, 32 * NT, a.Z ? "+store" : "", a.part_max ? "+pool" : "", X3 ? " x3" : (BF ? " bf16" : ""));
    const double rows = (double)a.rows_hint;
    ProfScope prof(name, 2.0 * rows * CIN * a.cout, rows * ((a.a_bf16 ? 2.0 : 4.0) * (double)CIN * cdiv(a.cout, CB) + (a.Z ? (a.z_bf16 ? 2.0 : 4.0) * a.cout : 0.0)), st);
    hipLaunchKernelGGL(kern, grid, dim3(NW * 64), lds, st, a);
    return check_launch("pw_gemm_kernel");
}

// the split kernels exist for the MFMA-bound shape (128 inputs, > 64 output columns per block) of the real point layers
constexpr int PW_X3_NW = 8;     // two waves per SIMD, one workgroup per CU (three bf16 images of the weight tile: 104 KB of LDS)
template <int CIN, int NT, int PRO, bool POOL>
// (the 64 -> 128 layers were built and measured on the split kernel too: 0.222 -> 0.194 ms per launch, -0.085 ms per step.  Not enabled: any change
// of rounding re-draws the chaotic T-Net gradient noise of tests/test_backward_gpu.py (a 3e-8 input perturbation moves those gradients by 0.02 .. 1 %,
// tests/diagnostics/x3_mode_diff.py), and this draw put one of its seven seeded cases at 2.8x its bar; the bars stay as they are.)
static constexpr bool pw_x3_built = CIN == 128 && NT == 4 && PRO == 1;

template <int CIN, int NT, int PRO, bool POOL>
static int launch_pw_x(const PwGemm &a, hipStream_t st)
{
    if (precision_is_f32()) {
        if constexpr (pw_x3_built<CIN, NT, PRO, POOL>) {
            if (precision_split() && !a.w_win_stride && a.uniform_rows == 0 && a.cout % (32 * NT) == 0 && (POOL ? !a.Z : a.Z != nullptr) && !a.bias && !a.identity_k &&
                (!a.part_sum || a.part_rows)) {       // the real point layers (not the T-Net FC rows)
                if constexpr (POOL) {
                    if (!a.part_amax) return launch_pw_y<CIN, NT, PRO, POOL, true, false, false, false, false, true, PW_X3_NW>(a, st);
                }
                return launch_pw_y<CIN, NT, PRO, POOL, true, false, false, false, true, true, PW_X3_NW>(a, st);
            }
        }
        // one-step-ahead operand reads: 2.3 % on the train step, 5.9 % on the eval forward in an interleaved same-box A/B
        // (tools/ab_pw_pipe.py); AMPNET_PW_PIPE=0 selects the plain K loop
        const char *pe = getenv("AMPNET_PW_PIPE");
        const bool pipe = !(pe && pe[0] == '0');
        if constexpr (POOL) {
            if (!a.part_amax)                                           // extremes only (eval forward): the ARG = false epilogue never touches part_amax
                return pipe ? launch_pw_y<CIN, NT, PRO, POOL, false, false, false, true, false>(a, st) : launch_pw_y<CIN, NT, PRO, POOL, false, false, false, false, false>(a, st);
        }
        return pipe ? launch_pw_y<CIN, NT, PRO, POOL, false, false, false, true>(a, st) : launch_pw_y<CIN, NT, PRO, POOL, false>(a, st);
    }
    const bool abf = a.a_bf16 != 0, zbf = a.z_bf16 != 0 && a.Z != nullptr;
    if (abf && zbf) return launch_pw_y<CIN, NT, PRO, POOL, true, true, true>(a, st);
    if (abf) return launch_pw_y<CIN, NT, PRO, POOL, true, true, false>(a, st);
    if (zbf) return launch_pw_y<CIN, NT, PRO, POOL, true, false, true>(a, st);
    return launch_pw_y<CIN, NT, PRO, POOL, true>(a, st);
}

// the (prologue, pool) variants each shape is actually used with; anything else is an argument error
template <int CIN, int NT>
static int launch_pw(const PwGemm &a, hipStream_t st)
{
    const int pro = a.pro_scale ? (a.drop_p > 0.f ? 2 : 1) : 0;
    const bool pool = a.part_max != nullptr;
    if (pool) {
        if constexpr (CIN == 128 && NT == 4) {
            if (pro == 1) return launch_pw_x<CIN, NT, 1, true>(a, st);
        }
        return fail(AMPNET_E_ARG, "pw_gemm: max-pool epilogue is built for cin 128, >64 columns, BatchNorm+ReLU prologue");
    }
    if (pro == 2) {
        if constexpr ((CIN == 128 && NT == 2) || (CIN == 64 && NT == 1)) return launch_pw_x<CIN, NT, 2, false>(a, st);
        return fail(AMPNET_E_ARG, "pw_gemm: dropout prologue is built for cin 128 / 33..64 columns and cin 64 / <= 32 columns");
    }
    return pro ? launch_pw_x<CIN, NT, 1, false>(a, st) : launch_pw_x<CIN, NT, 0, false>(a, st);
}

// lanes per slot for the per-workgroup statistics of a layer with one column block per row block: at most 512 workgroups (two per CU of
// the MI355X; on another part the surplus queues, the result does not change), never more than a slot has blocks of rows
PwStatPlan pw_gemm_stat_plan(int Q, int chunks, int n_slots, int max_lanes)
{
    PwStatPlan p;
    const long items = (long)Q * chunks;                      // blocks of rows in all
    int lanes = items < max_lanes ? (int)items : max_lanes;
    if (lanes < n_slots) lanes = n_slots;                     // every slot needs a lane (one that finds no rows writes an empty partial)
    p.lanes = lanes;
    p.parts = cdiv(lanes, n_slots) * n_slots;
    p.direct = cdiv(Q, n_slots) * chunks == 1;                // every slot is ONE block of rows: the workgroup's statistics are the slot's
    return p;
}

// the split kernels hold one workgroup per CU (three weight images in LDS): a persistent grid is 256 workgroups over the column blocks
int pw_gemm_stat_lane_cap(int cin, int cout)
{
    if (precision_split() && cin == 128 && cout > 64 && cout % 128 == 0) return 256 / (cout / 128);
    return 512;
}

int pw_gemm(const PwGemm &a, hipStream_t st)
{
    AMPNET_REQUIRE(a.A && a.W && (a.win_off || a.uniform_rows > 0), "pw_gemm: null pointer");
    AMPNET_REQUIRE(!a.part_rows || (a.part_sum && a.stat_lanes >= a.n_slots && a.stat_lanes <= 2048), "pw_gemm: per-workgroup statistics need part_sum and a lane plan");
    AMPNET_REQUIRE(!a.pfin.part.sum || (a.part_rows && a.pro_scale && a.pfin.part.sq && a.pfin.part.rows && a.pfin.part.parts >= a.n_slots && a.pfin.part.parts % a.n_slots == 0 && a.pfin.layer.gamma &&
                                   a.pfin.layer.beta && a.pfin.out.scale && a.pfin.out.shift && a.pfin.out.mean && a.pfin.out.invstd && a.pfin.out.smean && a.pfin.out.suvar && a.pfin.part.sum != a.part_sum &&
                                   a.pfin.part.rows != a.part_rows && (a.cin == 64 || a.cin == 128) && !a.w_win_stride && a.pfin.part.parts / a.n_slots <= 1024),
                   "pw_gemm: consumer-side BatchNorm finalize needs per-workgroup statistics, the producer's partials in buffers of their own and every output array");
    AMPNET_REQUIRE((!a.pfin.part.sum && !a.fin.out.scale) || bn_fwd_in_kernel(a.part_rows != nullptr), "pw_gemm: a BatchNorm is finished in the kernel from batch statistics, and not the global batch's");
    AMPNET_REQUIRE(!a.fin.out.scale || (a.part_rows && a.stat_lanes == a.n_slots && a.fin.layer.gamma && a.fin.layer.beta && a.fin.out.shift && cdiv(a.Q, a.n_slots) * a.chunks == 1),
                   "pw_gemm: in-kernel BatchNorm constants need one block of rows per slot");
    AMPNET_REQUIRE(a.Q >= 1 && a.chunks >= 1 && a.cout >= 1, "pw_gemm: bad sizes Q=%d chunks=%d cout=%d", a.Q, a.chunks, a.cout);
    AMPNET_REQUIRE(a.lda % 4 == 0 && (a.w_win_stride != 0 || a.ldw % 4 == 0), "pw_gemm: lda/ldw must be multiples of 4");
    AMPNET_REQUIRE(a.n_slots >= 1 && (!a.perwin_slot_major || a.Q % a.n_slots == 0), "pw_gemm: Q %% n_slots != 0");
    AMPNET_REQUIRE((a.part_sum == nullptr) == (a.part_sq == nullptr), "pw_gemm: part_sum/part_sq must come together");
    AMPNET_REQUIRE(!a.part_max || a.part_amax || (precision_is_f32() && !a.part_sum),
                   "pw_gemm: the pool epilogue without argmax rows is the fp32 eval form (no statistics)");
    AMPNET_REQUIRE(!(a.a_bf16 || a.z_bf16) || !precision_is_f32(), "pw_gemm: bf16 tensors need a bf16 precision mode");
    AMPNET_REQUIRE(!a.a_bf16 || a.lda % 8 == 0, "pw_gemm: bf16 A needs lda %% 8 == 0");
    int nt = a.cout > 64 ? 4 : (a.cout > 32 ? 2 : 1);
    // tiny problems (the T-Net FC layers: nine blocks of 64 rows): narrower column blocks = more workgroups, each staging a
    // smaller weight tile -- they are bound by that staging latency, not by the matrix cores
    while (nt > 1 && !a.part_max && !(a.drop_p > 0.f) && (long)a.Q * a.chunks * cdiv(a.cout, 32 * nt) < 128) nt >>= 1;
    switch (a.cin) {
    case 64:
        if (nt == 4) return launch_pw<64, 4>(a, st);
        if (nt == 2) return launch_pw<64, 2>(a, st);
        return launch_pw<64, 1>(a, st);
    case 128:
        if (nt == 4) return launch_pw<128, 4>(a, st);
        if (nt == 2) return launch_pw<128, 2>(a, st);
        return launch_pw<128, 1>(a, st);
    case 256:
        if (nt == 4) return launch_pw<256, 4>(a, st);
        if (nt == 2) return launch_pw<256, 2>(a, st);
        return launch_pw<256, 1>(a, st);
    default:
        return fail(AMPNET_E_ARG, "pw_gemm: cin=%d not in {64,128,256}", a.cin);
    }
}

}  // namespace ampnet

#ifdef AMPNET_PW_STAMPS
extern "C" int ampnet_debug_pw_stamps(unsigned long long *host_out, int max_entries)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    const size_t n = (size_t)(max_entries < 4096 ? max_entries : 4096);
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(ampnet::g_pw_stamps), n * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
