// Dense pixel-level matching (AEM:61-89, 178-227) on the fp16 matrix pipe with fp32-equivalent products.
//
// Every fp32 value x (scaled by 2^10) is split into hi = fp16(x') and lo = fp16(x' - hi): hi + lo represents x' to 2^-22 relative
// (two 11-bit significands; typically 2^-23), and q.r = qh.rh + qh.rl + ql.rh (+ a ql.rl term < 2^-22 |q||r| that is dropped)
// accumulates in fp32 inside v_mfma_f32_32x32x16_f16.  The reference pixel's -|r|^2/2 rides along in three spare k-slots of the hi
// plane (K = 100 pads to 112 anyway), so one accumulator holds 2^20 * (q.r - |r|^2/2) and the min over reference pixels becomes a max
// over raw accumulators.  |q|^2 and the 5e4 wrong-label padding (AEM:84-88) are applied per query pixel at the end: with one-hot
// labels min_j(d_j + 5e4 wrong[j,o]) = min(own_o, 5e4 + min_{o' != o} own_o').
//
// dense_prune_kernel evaluates the qh.rh product everywhere and the two cross products only where they can matter (see its header):
// about 40 % of the matrix instructions of evaluating all three everywhere, for the same result.
//
// This kernel only runs when (a) every scaled value fits fp16 and (b) every kept reference pixel is right for
// exactly one object; both facts are device flags, and the exact-fp32 kernels of correlation.hip take over on
// the same stream otherwise (each side checks the flag itself: no host round trip).
#include <atomic>
#include <type_traits>

#include "aoc_common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SP_KS = 7;                       // k-steps of 16 halves: 112 slots = 100 channels + 3 norm slots + pad
constexpr int SP_K = SP_KS * 16;
constexpr int SP_HALF = SP_KS * 2;             // 16-byte chunks per plane: per k-step [k0-7][k8-15]
constexpr int SP_REC = 2 * SP_HALF;            // 16-byte chunks per record: the hi plane (14 chunks), then the lo plane
constexpr int SP_NORM_SLOT = 100;              // slots 100..102 of the hi plane: the three fp16 pieces of -16 |r|^2
                                               // slots 104, 105 of the hi plane are reserved and zero
constexpr float SP_SCALE = 1024.0f;            // 2^10
constexpr float SP_QCONST = 32768.0f;          // query-side value of the norm slots: 2^15 * (-16 |r|^2) = -2^19 |r|^2
constexpr float SP_UNSCALE = -1.0f / 524288.0f;   // d - |q|^2 = -2^-19 * acc
constexpr int SP_TILE = 32;                    // reference pixels per MFMA tile
constexpr int SP_NB_HI = 8;                    // tiles per staged chunk (hi planes only)
constexpr int SP_NQ = 2;                       // 32-pixel query tiles per wave (stationary B operands in registers)
constexpr int SP_NW = 8;                       // waves per workgroup of dense_prune_kernel
constexpr int64_t SP_ROWS_PER_BLOCK = SP_NW * SP_NQ * 32;      // query pixels per workgroup

static_assert(SP_NORM_SLOT + 4 <= SP_K && SP_NORM_SLOT / 16 == SP_KS - 1 && (SP_NORM_SLOT % 16) + 4 <= 8, "norm slots live in the low half of the last k-step");

// ------------------------------------------------------------------------------------------
// fp32 rows -> split records (+ |x|^2).  One thread per (row, k-step).  Record = hi plane (14 x 16 B: per k-step [k0-7][k8-15]), then the
// lo plane in the same order; hi-plane slots 100..102 = the three fp16 pieces of -16 |x|^2, slot 103 = an upper bound of the lo plane's norm.
//
// TILED: the same chunks in the order a wave consumes them as MFMA B operands -- per 32-row tile, per plane, per k-step the 64 chunks
// [k-half h][row j] (1 KiB: ONE fully coalesced wave load per operand, no transposition on the consumer's side).  The buffer holds whole
// tiles; rows past n are written as zeros.  Threads: j fastest, so that a half wave writes 512 consecutive bytes.
template <bool TILED>
__global__ __launch_bounds__(256) void split_rows_kernel(const float *__restrict__ x, int64_t n, int C, uint4 *__restrict__ rec,
                                                          float *__restrict__ sqnorm, int32_t *__restrict__ overflow) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t row;
    int ks;
    if (TILED) {
        const int64_t tile = idx / (SP_KS * 32);
        const int rem = (int)(idx - tile * (SP_KS * 32));
        ks = rem >> 5;
        row = tile * 32 + (rem & 31);
        if (tile * 32 >= n) return;
    } else {
        row = idx / SP_KS;
        ks = (int)(idx - row * SP_KS);
        if (row >= n) return;
    }
    const bool live = row < n;                    // TILED: the last tile's rows past n are zero records
    const float *xr = x + (size_t)(live ? row : n - 1) * C;
    _Float16 hi[16], lo[16];
    bool bad = false;
    {
        // the k-step's 16 channels as four float4 loads issued together (clamped index, zero selected past the channels)
        const int c4k = C >> 2;
        float4 kv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) kv[q] = reinterpret_cast<const float4 *>(xr)[min(ks * 4 + q, c4k - 1)];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool in = ks * 4 + q < c4k;
            const float e4[4] = {kv[q].x, kv[q].y, kv[q].z, kv[q].w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float v = in ? e4[u] * SP_SCALE : 0.0f;
                bad |= !(fabsf(v) <= 65000.0f);
                hi[q * 4 + u] = (_Float16)v;
                lo[q * 4 + u] = (_Float16)(v - (float)hi[q * 4 + u]);
            }
        }
    }
    if (ks == SP_KS - 1) {
        float s = 0.0f, sl = 0.0f;
        // the whole row as 25 float4 loads issued together (a scalar loop is one dependent round trip per channel); the additions keep
        // the sequential order t = 0 .. C-1
        float4 rv[SP_NORM_SLOT / 4];
        const int c4n = C >> 2;
#pragma unroll
        for (int t4 = 0; t4 < SP_NORM_SLOT / 4; ++t4) rv[t4] = reinterpret_cast<const float4 *>(xr)[t4 < c4n ? t4 : c4n - 1];
#pragma unroll
        for (int t4 = 0; t4 < SP_NORM_SLOT / 4; ++t4) {
            if (t4 < c4n) {
                const float e[4] = {rv[t4].x, rv[t4].y, rv[t4].z, rv[t4].w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    s += e[u] * e[u];
                    const float v = e[u] * SP_SCALE;
                    const float hv = (float)(_Float16)v;                            // the hi value of the channel, as its own thread stores it
                    const float l = (float)(_Float16)(v - hv);                      // ... and the lo value
                    sl += l * l;
                }
            }
        }
        if (sqnorm && live) sqnorm[row] = s;
        bad |= !(s <= 4000.0f);
        const float p = -16.0f * s;
        const _Float16 p1 = (_Float16)p;
        const _Float16 p2 = (_Float16)(p - (float)p1);
        const _Float16 p3 = (_Float16)((p - (float)p1) - (float)p2);
        hi[SP_NORM_SLOT % 16] = p1;
        hi[SP_NORM_SLOT % 16 + 1] = p2;
        hi[SP_NORM_SLOT % 16 + 2] = p3;
        // slot 103: an upper bound of the Euclidean norm of the row's lo plane (the rescoring margin of the dense kernel); the
        // query side multiplies it by zero
        hi[SP_NORM_SLOT % 16 + 3] = (_Float16)(sqrtf(sl) * 1.002f + 1e-6f);
        // slots 104, 105 are reserved and zero
    }
    if (bad && live) atomicOr(overflow, 1);
    union { _Float16 h[32]; uint4 q[4]; } u;
#pragma unroll
    for (int e = 0; e < 16; ++e) { u.h[e] = hi[e]; u.h[16 + e] = lo[e]; }
    if (TILED) {
        if (!live) u.q[0] = u.q[1] = u.q[2] = u.q[3] = make_uint4(0, 0, 0, 0);
        uint4 *dst = rec + ((size_t)(row >> 5) * 2 * SP_KS + ks) * 64 + (row & 31);
        dst[0] = u.q[0];
        dst[32] = u.q[1];
        dst[SP_KS * 64] = u.q[2];
        dst[SP_KS * 64 + 32] = u.q[3];
    } else {
        uint4 *dst = rec + (size_t)row * SP_REC + ks * 2;
        dst[0] = u.q[0];
        dst[1] = u.q[1];
        dst[SP_HALF] = u.q[2];
        dst[SP_HALF + 1] = u.q[3];
    }
}

// ------------------------------------------------------------------------------------------
// Plan: the per-object row lists of label prep cut into 32-row tiles (object-pure, -1 padded), the tile count, and
// the one-hot check.  gate[0] |= overflow | (some kept row is not right for exactly one object).
__global__ __launch_bounds__(256) void split_plan_kernel(const int32_t *__restrict__ obj_rows, const int32_t *__restrict__ counts,
                                                          const int32_t *__restrict__ obj_offsets, int n_obj, int64_t n,
                                                          const uint32_t *__restrict__ right_bits, const uint32_t *__restrict__ wrong_bits,
                                                          const int32_t *__restrict__ overflow, const uint4 *__restrict__ prec,
                                                          int64_t tile_capacity, int32_t *__restrict__ tile_rows,
                                                          int32_t *__restrict__ tile_obj, int32_t *__restrict__ n_tiles,
                                                          int32_t *__restrict__ gate, uint32_t *__restrict__ pmax_bits) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float sq = 0.0f, ln = 0.0f;
    if (e < n) {
        const uint32_t mask = (n_obj >= 32) ? 0xffffffffu : ((1u << n_obj) - 1u);
        const uint32_t right = right_bits[e];
        if (right & AOC_ROW_KEPT_BIT) {
            const uint32_t r = right & mask, nw = ~wrong_bits[e] & mask;
            if (__popc(r) != 1 || nw != r) atomicOr(gate, 1);
            // |r|^2 back from the record's norm slots (three fp16 pieces of -16 |r|^2)
            union { uint4 q; _Float16 hh[8]; } u;
            u.q = prec[(size_t)e * SP_REC + (SP_KS - 1) * 2];
            sq = -((float)u.hh[SP_NORM_SLOT % 16] + (float)u.hh[SP_NORM_SLOT % 16 + 1] + (float)u.hh[SP_NORM_SLOT % 16 + 2]) * 0.0625f;
            ln = (float)u.hh[SP_NORM_SLOT % 16 + 3];
        }
    }
    // largest squared norm among the kept reference pixels (non-negative floats order like their bit patterns)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sq = __builtin_fmaxf(sq, __shfl_xor(sq, d));
        ln = __builtin_fmaxf(ln, __shfl_xor(ln, d));
    }
    // one atomic per wave only while the wave can still raise the maximum (thousands of atomics on two addresses serialise: most of this
    // kernel's 64 us): a relaxed device-scope read first, the atomic only if the wave's value is larger than what is already there
    if (aoc_lane() == 0 && sq > 0.0f && __float_as_uint(sq) > __hip_atomic_load(pmax_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(pmax_bits, __float_as_uint(sq));
    if (aoc_lane() == 0 && ln > 0.0f && __float_as_uint(ln) > __hip_atomic_load(pmax_bits - 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(pmax_bits - 2, __float_as_uint(ln));      // gate[1]: largest lo-plane norm
    if (e == 0 && overflow && *overflow) atomicOr(gate, 1);
    const int64_t t = e / SP_TILE;
    const int i = (int)(e - t * SP_TILE);
    if (t >= tile_capacity) return;
    int64_t base = 0;
    int obj = -1, local = 0;
    for (int o = 0; o < n_obj; ++o) {
        const int64_t nt = (counts[o] + SP_TILE - 1) / SP_TILE;
        // an object's tiles in DESCENDING row order: the newest pool frame first -- that is where a video's best matches usually are, and an
        // early good match tightens the bounds for everything after it
        if (obj < 0 && t < base + nt) { obj = o; local = (int)(nt - 1 - (t - base)); }
        base += nt;
    }
    if (e == 0) *n_tiles = (int32_t)base;
    // a partial last tile is filled up with copies of its first row (a duplicate cannot change a maximum): no padding values anywhere
    int32_t id = -1;
    if (obj >= 0) {
        const int pos = local * SP_TILE + i;
        id = obj_rows[obj_offsets[obj] + (pos < counts[obj] ? pos : local * SP_TILE)];
    }
    tile_rows[e] = id;
    if (i == 0) tile_obj[t] = obj;
}

// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float max16(const f32x16 &a) {
    float m0 = __builtin_fmaxf(__builtin_fmaxf(a[0], a[1]), a[2]);
    float m1 = __builtin_fmaxf(__builtin_fmaxf(a[3], a[4]), a[5]);
    float m2 = __builtin_fmaxf(__builtin_fmaxf(a[6], a[7]), a[8]);
    float m3 = __builtin_fmaxf(__builtin_fmaxf(a[9], a[10]), a[11]);
    float m4 = __builtin_fmaxf(__builtin_fmaxf(a[12], a[13]), a[14]);
    m0 = __builtin_fmaxf(__builtin_fmaxf(m0, m1), m2);
    m3 = __builtin_fmaxf(__builtin_fmaxf(m3, m4), a[15]);
    return __builtin_fmaxf(m0, m3);
}

// float <-> unsigned with the same order (atomicMax on the encoding = max on the floats); every encoded finite value or infinity
// is > 0, so a zeroed word means "nothing yet"
__device__ __forceinline__ uint32_t ord_enc(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_dec(uint32_t u) {
    if (u == 0u) return -INFINITY;
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ uint32_t load_relaxed(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ unsigned long long g_prune_stats[8];    // (tile, query tile) pairs tested / rescored, tiles with any rescoring, tiles; [4..7] reserved (0)

// LDS-DMA: 64 lanes x 16 bytes (or 4 bytes) from per-lane global addresses to the LDS bytes [lds_dst + 16 lane, +16).  Written in asm so
// that hipcc neither counts nor drains it: completion is the kernel's own vmcnt arithmetic (see the step loop).
__device__ __forceinline__ void glds16(const void *gsrc, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void glds4(const void *gsrc, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

constexpr int SP_NBUF = 2;                                        // chunk buffers in LDS
// LDS layout of a workgroup.  A staged row is its hi plane only (224 B of the 448-byte record), rows unpadded
constexpr int SP_ROW_CHUNKS = SP_HALF, SP_ROW_BYTES = SP_ROW_CHUNKS * 16, SP_TILE_BYTES = SP_TILE * SP_ROW_BYTES;      // a staged row / tile
constexpr int SP_CHUNK_BYTES = SP_NB_HI * SP_TILE_BYTES;          // 57344: eight tiles x 32 rows x 224 B
// row ids: 3 slots x 256 ids (the rescoring reads the CURRENT chunk's ids while the next two are in the ring)
constexpr int SP_IDS_SLOTS = 3, SP_IDS_SLOT_BYTES = 1024;
constexpr int SP_IDS_OFF = SP_NBUF * SP_CHUNK_BYTES;
constexpr int SP_OBJ_OFF = SP_IDS_OFF + SP_IDS_SLOTS * SP_IDS_SLOT_BYTES;
constexpr int SP_BND_OFF = SP_OBJ_OFF + 4 * 256;                  // before it: 4 slots x 64 tile objects (8 used)
constexpr int SP_LDS_BYTES = SP_BND_OFF + SP_NW * SP_NQ * 256;    // per (wave, query tile): 64 published bounds
static_assert(SP_NQ == 2 && SP_NW == 8 && SP_NB_HI == 8 && SP_LDS_BYTES == 122880,
              "the step structure of dense_prune_kernel is written for 8 hi-plane tiles x 2 query tiles x 8 waves; 120 KiB per workgroup");
constexpr int SP_TILE_SLACK = 2;                                  // the plan always holds an empty tile after the last one

// Coarse-then-rescore.  Block = 8 waves x 2 query tiles (512 query pixels; both planes of their records are the stationary B
// operands, 112 VGPR); the object-sorted reference tiles stream through two LDS chunk buffers (8 tiles each, hi planes only; A operands).
// Work list = (query blocks, tile splits), walked by a grid of resident workgroups (see the item loop).  Per (reference tile, query tile) ONE pass of 7 MFMAs gives
// coarse = 2^20 (qh.rh - |r|^2/2); the exact three-product value differs from it by the qh.rl + ql.rh terms, bounded by
// eps(q) = 2^10 |q| max|r| (1 + margins): a pair whose coarse value plus eps is below the best EXACT value already known for that
// (query pixel, object) cannot hold the maximum and is skipped; any other pair gets the 14 MFMAs of the two cross terms added onto the
// same accumulators, which is then exactly the three-product value (the reference tile's lo plane, which only these 5 % of the pairs
// read, is fetched from the records in global memory at that point, see the rescoring path).  The best
// exact values live in gbest[pixel][object] (atomicMax on an order-preserving encoding) and are shared by all splits and by the
// workgroups of later rounds, so the bound tightens after the first few tiles anywhere on the chip.  The true maximum always survives
// (coarse + eps >= exact >= every bound) and its value does not depend on what else was evaluated: the result is deterministic
// although the set of rescored tiles is not.
//
// Data movement: the chunk of step s + 1 is fetched by LDS-DMA while step s computes (no staging registers, no ds_write pass); its row
// ids (and the tiles' objects) were themselves DMA'd one step earlier, and the bounds other workgroups published come in the same
// way.  LDS rows are unpadded (224 B, the 14 hi chunks of the 448-byte record); chunk c of row r sits at position
// c ^ ((r >> 3) & 1), which makes every ds_read_b128 of an A fragment conflict-free (derivation at SWZ_MASK) -- the swizzle is
// applied on the SOURCE address of the DMA, whose destination is lane-linear.  The transfers are asm statements that hipcc neither counts
// nor drains; one vmcnt(0) + barrier per step publishes them.
//
// Why hi planes only (profiles/dense_hi_ring_ab.txt): what a step costs apart from its tiles -- issuing the 7 transfers per wave, vmcnt(0), the
// bound read-back, the barrier at which the waves' rescoring imbalance meets -- was 850 of ~2 290 cycles per tile with four-tile steps; the lo
// plane was half of every transfer and of the ring and is read by the rescoring path only.  The same 2 x 56 KiB now hold eight tiles per step.
// LDS per workgroup: 2 x 57 344 (ring) + 3 x 1 024 (row ids: the chunk in use, the one being fetched, the one after) + 4 x 256 (tile objects)
// + 16 x 256 (bounds) = 120 KiB.  The published bounds are taken in once per step as before, i.e. every eight tiles now: the rescored share of
// the bench's R = 6 pools went from 4.9 to 5.1 %; a refresh half way through the step brought it back and cost more than it saved (same file).
//
// Measured and rejected, and no longer in this file (the code is in the history up to commit d00d738; the verdicts are in STATUS.md,
// profiles/r05_dense_experiments.txt, profiles/r06_dense_experiments.txt and profiles/dense_hi_ring_ab.txt): a checkpoint after 3 / 4 of the
// 7 k-steps (stops 26 % / 40 % of the pairs of the bench's R = 6 pools, same results, and the kernel is 16 % / 13 % SLOWER: the wave has to wait
// for its own MFMA results in the middle of every tile, and with two waves per SIMD nothing hides that wait); one wave per SIMD with four query
// tiles per wave (a wash in the bench); workgroups of four waves, with four or two tiles per chunk; the ring of whole records, four tiles per
// chunk (the A / B partner of the hi-plane ring).
//
// One template parameter that never varies is kept on purpose: a template instantiation is emitted behind the plain kernels of this file, where the
// measured kernel sat.  Written as a plain function the same instructions land in front of them and the bench loses 1-2 % (427.8 / 430.6 / 429.4
// against 421.6 / 420.1 / 416.5 frames/s, the parent's library 427.9 / 426.2 / 426.1 in the same runs: profiles/variants_out_ab.txt, section 3).
template <int PLACE>
__global__ __launch_bounds__(SP_NW * 64, 1) void dense_prune_kernel(const uint4 *__restrict__ qrec, const float *__restrict__ q2, int64_t m,
                                                                     const uint4 *__restrict__ prec, const int32_t *__restrict__ tile_rows,
                                                                     const int32_t *__restrict__ tile_obj, const int32_t *__restrict__ n_tiles_ptr,
                                                                     const int32_t *__restrict__ gate, const uint32_t *__restrict__ pmax_bits,
                                                                     int n_obj, uint32_t *__restrict__ gbest, int q_tiled, int n_split) {
    if (*gate) return;
    extern __shared__ __attribute__((aligned(16))) uint4 lds4[];
    // Swizzle of the unpadded LDS rows: chunk c of row r sits at position c ^ ((r >> 3) & SWZ_MASK).  A ds_read_b128 is served in groups of 16 lanes
    // (rows {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of the tile, one k-half each) that must hit 16 different 16-byte columns of the 256-byte bank
    // line.  224-byte rows: column = (14 r + position) mod 16 = (position - 2 r) mod 16; the eight residues of r mod 8 give the eight even
    // offsets, each shared by TWO rows of a group -- (r, r + 24) or (r, r + 8), with r >> 3 = 0 | 3 or 1 | 2 -- and bit 0 of the position, flipped
    // by bit 3 of the row, puts one of the two on the odd column (mask 1; positions 2 k and 2 k + 1 swap, so a row stays inside its 14 chunks).
    constexpr int SWZ_MASK = 1;
    constexpr int SP_DMA_PER_WAVE = SP_CHUNK_BYTES / 1024 / SP_NW;   // 7 wave-wide 1 KiB transfers per wave and chunk
    constexpr int W_ID0 = SP_NW / 2, W_OBJ = 1;                      // the waves that also fetch the row ids / the tiles' objects
    const uint32_t lds_base = (uint32_t)reinterpret_cast<uintptr_t>(lds4);
    const char *lds_bytes = reinterpret_cast<const char *>(lds4);

    // The work list: items (query block bx, tile split by), nbx x n_split of them, split-major.  The grid is G RESIDENT workgroups (one per CU
    // of the share of the stream's CUs that aoc_dense_split_sizing gives this kernel); workgroup w walks the items lin = w, w + G, w + 2 G, ...
    // Per item everything starts over: the stationary query operands, the LDS ring, the bounds (those live in gbest and are shared anyway).
    const int n_tiles = *n_tiles_ptr;
    const int ns = n_split;
    const int nbx = (int)((m + SP_ROWS_PER_BLOCK - 1) / SP_ROWS_PER_BLOCK), nb = nbx * ns;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned n_rescored = 0, n_any = 0, n_seen = 0;
#pragma unroll 1
    for (int lin = blockIdx.x; lin < nb; lin += gridDim.x) {
        // The lane index is made opaque once per item: what an item derives from it (operand addresses, the DMA plan, the fragment offsets) is then
        // computed inside the item and dies there, as in a kernel that runs one item; hoisted out of this loop those values stay live across the tile loop
        // and the kernel no longer fits the 256 registers of two waves per SIMD (it spills).
        int lane = aoc_lane();
        asm volatile("" : "+v"(lane));
        const int col = lane & 31, h = lane >> 5;
        const float pmax = sqrtf(__uint_as_float(*pmax_bits)) * 1.001f;
        const float plmax = __uint_as_float(*(pmax_bits - 2));
        // XCD-aware item -> (query block, tile split) map: workgroups are dealt round-robin to the 8 XCDs, each with its own
        // L2; give every XCD a contiguous range of the (split-major) work list so that the ~nbx workgroups that stream the
        // same reference tiles share one L2 instead of pulling them through all eight.  G is a multiple of 8 (when it is 8 or more), so
        // lin & 7 is the same for every item of a workgroup: it stays inside its XCD's range.
        int bx, by;
        {
            const int xcd = lin & 7, slot = lin >> 3, q = nb >> 3, r = nb & 7;
            const int v = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
            by = v / nbx;
            bx = v - by * nbx;
        }
        // split `by` owns the tiles by, by + ns, by + 2 ns, ...: every split sees the same mix of objects (small objects rescore far more often
        // than the background; contiguous ranges would leave all of that work to the last splits, i.e. to one XCD)
        if (by >= n_tiles) continue;              // (uniform over the workgroup: no barrier is skipped by a part of it)
        const int n_mine = (n_tiles - by + ns - 1) / ns;
        const int n_chunks = (n_mine + SP_NB_HI - 1) / SP_NB_HI;

        const int64_t wave_row0 = (int64_t)bx * (SP_NW * SP_NQ * 32) + (int64_t)wave * (SP_NQ * 32);

        // ---- stationary query operands (both planes) and the per-pixel rescoring margin
        f16x8 bh[SP_NQ][SP_KS], bl[SP_NQ][SP_KS];
        float eps[SP_NQ];
        bool valid[SP_NQ];
#pragma unroll
        for (int iq = 0; iq < SP_NQ; ++iq) {
            const int64_t row = wave_row0 + iq * 32 + col;
            valid[iq] = row < m;
            // row-major records: chunk (plane, ks, h) of row r at r * 28 + plane * 14 + ks * 2 + h; tile-major (aoc_split_rows_tiled): per
            // (32-row tile, plane, ks) the 64 chunks [h][row % 32] -- one coalesced 1 KiB wave load per operand
            const int64_t rr = valid[iq] ? row : 0;
            const uint4 *r = q_tiled ? qrec + (size_t)(rr >> 5) * (2 * SP_KS * 64) + h * 32 + (rr & 31) : qrec + (size_t)rr * SP_REC + h;
            const int ks_step = q_tiled ? 64 : 2, plane_step = q_tiled ? SP_KS * 64 : SP_HALF;
#pragma unroll
            for (int ks = 0; ks < SP_KS; ++ks) {
                uint4 u = r[ks * ks_step], v = r[plane_step + ks * ks_step];
                if (!valid[iq]) { u = make_uint4(0, 0, 0, 0); v = make_uint4(0, 0, 0, 0); }
                bh[iq][ks] = __builtin_bit_cast(f16x8, u);
                bl[iq][ks] = __builtin_bit_cast(f16x8, v);
            }
            // norm slots: the query side holds the constant 2^15 (its own norm pieces sit in the record for when the
            // frame later joins the pool); everything else past the channels is zero on both planes
            const float ql_own = (float)bh[iq][SP_KS - 1][SP_NORM_SLOT % 16 + 3];      // lanes h == 0: the norm of the query pixel's own lo plane
            if (h == 0) {
                bh[iq][SP_KS - 1][SP_NORM_SLOT % 16 + 3] = (_Float16)0.0f;
                bh[iq][SP_KS - 1][SP_NORM_SLOT % 16] = (_Float16)SP_QCONST;
                bh[iq][SP_KS - 1][SP_NORM_SLOT % 16 + 1] = (_Float16)SP_QCONST;
                bh[iq][SP_KS - 1][SP_NORM_SLOT % 16 + 2] = (_Float16)SP_QCONST;
            } else {
                // slots 104 / 105 (reserved, zero in records written by this build): multiplied by zero whatever an older record holds there
                bh[iq][SP_KS - 1][0] = (_Float16)0.0f;
                bh[iq][SP_KS - 1][1] = (_Float16)0.0f;
            }
            // |exact - coarse| = |qh.rl + ql.rh| <= |qh| |rl| + |ql| |rh| (Euclidean norms of the planes, Cauchy-Schwarz) with |qh| <= 2^10 |q|
            // (1 + 2^-11), the lo norms as the records carry them (rounded up) and the maxima over the kept reference pixels, plus the
            // roundings of 14 more accumulations
            const float qn = valid[iq] ? sqrtf(q2[row]) : 0.0f;
            const float ql = valid[iq] ? __shfl(ql_own, col) : 0.0f;
            // (+ 0.0f: the place of the removed checkpoint's term.  The compiler may not fold it (-0), and without it the prologue is scheduled
            // differently; it stays so that the instruction stream is the measured one)
            eps[iq] = 1026.0f * (qn * plmax + ql * pmax) + 8.0f * pmax * pmax + 0.0f + 8.0f;
        }

        // ---- DMA plan of this wave: transfer k of a chunk fills the LDS slots [64 (7 wave + k), +64); slot j holds row j / 14, position j % 14.
        // Packed per transfer: row of the chunk (0..255) in the high half, source byte offset of that position's chunk in the low half.
        uint32_t dma_plan[SP_DMA_PER_WAVE];
#pragma unroll
        for (int k = 0; k < SP_DMA_PER_WAVE; ++k) {
            const int j = (wave * SP_DMA_PER_WAVE + k) * 64 + lane;
            const int r = j / SP_ROW_CHUNKS, pos = j - r * SP_ROW_CHUNKS;
            dma_plan[k] = ((uint32_t)r << 16) | (uint32_t)((pos ^ ((r >> 3) & SWZ_MASK)) * 16);
        }
        const char *prec_bytes = reinterpret_cast<const char *>(prec);
        auto dma_meta = [&](int chunk) {            // row ids (one wave) and tile objects (one wave) of a chunk -> their rings
            // tile i of the split is tile by + i ns of the plan; past the end everything reads the (always present) empty tile n_tiles
            const int i0 = chunk * SP_NB_HI;
            // eight tiles x 32 ids = 1 KiB: ONE 16-byte transfer of one wave (lane -> tile lane / 8, ids 4 (lane % 8) .. + 3)
            if (wave == W_ID0) {
                const int t = min(by + (i0 + (lane >> 3)) * ns, n_tiles);
                glds16(tile_rows + (size_t)t * SP_TILE + (lane & 7) * 4, lds_base + SP_IDS_OFF + (chunk % SP_IDS_SLOTS) * SP_IDS_SLOT_BYTES);
            }
            if (wave == W_OBJ) glds4(tile_obj + min(by + (i0 + (lane & (SP_NB_HI - 1))) * ns, n_tiles), lds_base + SP_OBJ_OFF + (chunk & 3) * 256);
        };
        auto dma_rows = [&](int chunk) {            // the chunk's hi planes -> buffer chunk % 2 (its ids must have landed and been published)
            const int32_t *ids = reinterpret_cast<const int32_t *>(lds_bytes + SP_IDS_OFF + (chunk % SP_IDS_SLOTS) * SP_IDS_SLOT_BYTES);
            const uint32_t dst = lds_base + (uint32_t)(chunk % SP_NBUF) * SP_CHUNK_BYTES + (uint32_t)(wave * SP_DMA_PER_WAVE) * 1024u;
            int id[SP_DMA_PER_WAVE];
#pragma unroll
            for (int k = 0; k < SP_DMA_PER_WAVE; ++k) id[k] = ids[dma_plan[k] >> 16];      // all LDS reads before the first (ordering) asm statement
#pragma unroll
            for (int k = 0; k < SP_DMA_PER_WAVE; ++k)
                glds16(prec_bytes + (size_t)(uint32_t)max(id[k], 0) * (SP_REC * 16) + (dma_plan[k] & 0xffffu), dst + (uint32_t)k * 1024u);
        };

        // best[iq]: best exact value this lane has produced for the current object; shared[iq]: the best anybody has published
        float best[SP_NQ], shared[SP_NQ];
        uint32_t grow[SP_NQ];                          // grow: word index of (pixel, object 0) in gbest (pixel 0 for rows past the end)
#pragma unroll
        for (int iq = 0; iq < SP_NQ; ++iq) {
            grow[iq] = valid[iq] ? (uint32_t)(wave_row0 + iq * 32 + col) * (uint32_t)n_obj : 0u;
            best[iq] = INFINITY;
            shared[iq] = INFINITY;
        }
        int cur = -1;
        // what the other workgroups have published for the current object: one 4-byte transfer per query tile into this wave's own LDS
        // words, read back one step later (device-scope load: the values come from L2, not from this CU's vector cache)
        auto dma_bound = [&]() {
#pragma unroll
            for (int iq = 0; iq < SP_NQ; ++iq) {
                unsigned keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off sc1\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(gbest + grow[iq] + max(cur, 0)), "s"(lds_base + SP_BND_OFF + (uint32_t)(wave * SP_NQ + iq) * 256u) : "memory");
            }
        };
        auto switch_object = [&](int o) {
            cur = o;
            uint32_t u[SP_NQ];
#pragma unroll
            for (int iq = 0; iq < SP_NQ; ++iq) u[iq] = load_relaxed(gbest + grow[iq] + cur);
#pragma unroll
            for (int iq = 0; iq < SP_NQ; ++iq) {
                best[iq] = valid[iq] ? -INFINITY : INFINITY;         // rows past the end never ask for a rescoring
                shared[iq] = valid[iq] ? ord_dec(u[iq]) : INFINITY;
            }
        };

        // ---- prologue: meta of chunks 0 and 1, rows of chunk 0 (drained: once per workgroup)
        dma_meta(0);
        dma_meta(1);
        __builtin_amdgcn_s_waitcnt(0x0f70);                           // vmcnt(0)
        __builtin_amdgcn_s_barrier();
        dma_rows(0);
        __builtin_amdgcn_s_waitcnt(0x0f70);
        __builtin_amdgcn_s_barrier();

        // A fragment addressing: chunk index e + h (e even, compile time) of row (tile, col) sits at position (e & ~1) + (h ^ x),
        // x = (col >> 3) & 1: one per-lane byte offset covers it
        const int xs = (col >> 3) & SWZ_MASK;
        const uint32_t row_off = (uint32_t)col * SP_ROW_BYTES;
        const uint32_t sw0 = row_off + (uint32_t)((h ^ xs) * 16), sw2 = sw0 + 32u;
        auto frag = [&](const char *tile_base, int e) -> f16x8 {       // e: even chunk index (2 ks)
            const uint32_t off = ((e & 2) ? sw2 : sw0) + (uint32_t)((e & ~3) * 16);
            return __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4 *>(tile_base + off));
        };
        auto ks_of = [&](int kk) { return (kk + SP_KS - 1) % SP_KS; };  // norm slots first: partial sums stay small

        for (int s = 0; s < n_chunks; ++s) {
            // (a) prefetches for the next step: published bounds of the current object, meta of chunk s + 2, rows of chunk s + 1 (whose ids
            // the barrier that ended step s - 1 published)
            const int4 objs = *reinterpret_cast<const int4 *>(lds_bytes + SP_OBJ_OFF + (s & 3) * 256);
            const int4 objs_b = *reinterpret_cast<const int4 *>(lds_bytes + (s & 3) * 256 + SP_OBJ_OFF + 16);      // tiles 4..7
            const int bound_obj = cur;
            dma_bound();
            dma_meta(s + 2);
            dma_rows(s + 1);

            // (b) the eight tiles of chunk s
            const char *chunk_base = lds_bytes + (s % SP_NBUF) * SP_CHUNK_BYTES;
            const int n_here = min(SP_NB_HI, n_mine - s * SP_NB_HI);
            // the first two A fragments of a tile are requested while the previous tile's epilogue runs
            f16x8 pre0 = frag(chunk_base, 2 * ks_of(0)), pre1 = frag(chunk_base, 2 * ks_of(1));
            // the tiles' objects in one 64-bit scalar (objects are < 256): two SALU operations per tile instead of a chain of selects
            const uint32_t objs_lo = (uint32_t)__builtin_amdgcn_readfirstlane((objs.x & 0xff) | ((objs.y & 0xff) << 8) | ((objs.z & 0xff) << 16) | ((objs.w & 0xff) << 24));
            const uint32_t objs_hi = (uint32_t)__builtin_amdgcn_readfirstlane((objs_b.x & 0xff) | ((objs_b.y & 0xff) << 8) | ((objs_b.z & 0xff) << 16) | ((objs_b.w & 0xff) << 24));
            const uint64_t objs_packed = ((uint64_t)objs_hi << 32) | objs_lo;
            // the current chunk's row ids (the rescoring path addresses the lo planes in global memory with them)
            const int32_t *ids_now = reinterpret_cast<const int32_t *>(lds_bytes + SP_IDS_OFF + (s % SP_IDS_SLOTS) * SP_IDS_SLOT_BYTES);
#pragma unroll 1
            for (int t = 0; t < n_here; ++t) {
                const char *tile_base = chunk_base + t * SP_TILE_BYTES;
                const int o = (int)((objs_packed >> (8 * t)) & 0xffu);
                if (o != cur) switch_object(o);
                // coarse pass: 7 k-steps x 2 query tiles, A fragments two k-steps ahead through a ring of three
                f32x16 acc[SP_NQ];
#pragma unroll
                for (int iq = 0; iq < SP_NQ; ++iq)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[iq][r] = 0.0f;
                {
                    f16x8 af[3];
                    af[0] = pre0;
                    af[1] = pre1;
#pragma unroll
                    for (int kk = 0; kk < SP_KS; ++kk) {
                        if (kk + 2 < SP_KS) af[(kk + 2) % 3] = frag(tile_base, 2 * ks_of(kk + 2));
#pragma unroll
                        for (int iq = 0; iq < SP_NQ; ++iq)
                            acc[iq] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[kk % 3], bh[iq][ks_of(kk)], acc[iq], 0, 0, 0);
                    }
                    if (t + 1 < n_here) {
                        pre0 = frag(tile_base + SP_TILE_BYTES, 2 * ks_of(0));
                        pre1 = frag(tile_base + SP_TILE_BYTES, 2 * ks_of(1));
                    }
                }
                // which query tiles may hold a new maximum (wave-uniform)
                bool want[SP_NQ];
#pragma unroll
                for (int iq = 0; iq < SP_NQ; ++iq) {
                    const float cm = max16(acc[iq]);
                    want[iq] = __builtin_amdgcn_ballot_w64(cm + eps[iq] >= __builtin_fmaxf(best[iq], shared[iq])) != 0ull;
                }
                n_seen += 1;
                if (want[0] || want[1]) {
                    n_any += 1;
                    // the tile's lo plane comes from the records in global memory (L2 / Infinity Cache resident: every workgroup of the
                    // split streams the same tiles), once per tile for both query tiles -- seven 16-byte loads per lane, row = the CURRENT chunk's id
                    // (slot s % 3 of the id ring; dma_meta(s + 2) and dma_rows(s + 1) use the other two slots during this step) -- and is waited for
                    // right here with an explicit vmcnt(0).  Outstanding at that point: the seven loads; in front of them this step's LDS-DMA statements
                    // (2 bounds, up to 2 meta, 7 rows: asm that hipcc does not count) unless an earlier tile of the step has drained them already, and
                    // fire-and-forget atomics of earlier rescorings.  vmcnt retires in issue order, so any wait for the loads covers all of these:
                    // correct, and a rescoring early in a step waits for the next chunk to land as well (the end of the step waits for it anyway).  No
                    // LDS-DMA is issued between the loads and their use.  Why not hipcc's own counted waits in front of each MFMA (vmcnt(6) ... (0)): the
                    // two rescorings are separate branches, its wait insertion merges the paths behind them, cannot know that one of the two always
                    // runs, keeps the loads pending around the tile loop and drains vmcnt(0) -- i.e. this step's DMA -- in front of EVERY tile's
                    // decision.  The explicit wait costs a rescoring tile the ~100 cycles of the first LDS read and MFMA that could have overlapped.
                    // Register arrays are indexed by unrolled constants only.
                    f16x8 alg[SP_KS];
                    auto load_lo = [&]() {
                        const int id = ids_now[t * SP_TILE + col];
                        const uint4 *lo = reinterpret_cast<const uint4 *>(prec_bytes + (size_t)(uint32_t)max(id, 0) * (SP_REC * 16) + SP_HALF * 16) + h;
#pragma unroll
                        for (int kk = 0; kk < SP_KS; ++kk) alg[kk] = __builtin_bit_cast(f16x8, lo[2 * ks_of(kk)]);
                        __builtin_amdgcn_s_waitcnt(0x0f70);                 // vmcnt(0)
                    };
                    auto rescore = [&](auto iq_c) {
                        constexpr int iq = decltype(iq_c)::value;
                        // cross terms: acc += rh.ql + rl.qh (one chain of 14 MFMAs), then the exact maximum
                        n_rescored += 1;
                        f16x8 ah[3];
#pragma unroll
                        for (int kk = 0; kk < 2; ++kk) ah[kk] = frag(tile_base, 2 * ks_of(kk));
#pragma unroll
                        for (int kk = 0; kk < SP_KS; ++kk) {
                            if (kk + 2 < SP_KS) ah[(kk + 2) % 3] = frag(tile_base, 2 * ks_of(kk + 2));
                            acc[iq] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[kk % 3], bl[iq][ks_of(kk)], acc[iq], 0, 0, 0);
                            acc[iq] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alg[kk], bh[iq][ks_of(kk)], acc[iq], 0, 0, 0);
                        }
                        const float ex = max16(acc[iq]);
                        if (ex > best[iq]) {
                            best[iq] = ex;
                            if (ex > shared[iq]) atomicMax(gbest + grow[iq] + cur, ord_enc(ex));      // fire and forget
                        }
                    };
                    load_lo();
                    if (want[0]) rescore(std::integral_constant<int, 0>{});
                    if (want[1]) rescore(std::integral_constant<int, 1>{});
                }
            }

            // (c) this step's transfers have landed (they had the step's tiles of time).  The wave reads back its own bound words right away (its
            // own vmcnt(0) covers them) so that the lgkmcnt(0) below also retires those reads before the next step's transfer can overwrite
            // the words; then the barrier publishes the chunk and the row ids to the other waves.
            __builtin_amdgcn_s_waitcnt(0x0f70);          // vmcnt(0)
            uint32_t seen[SP_NQ];
#pragma unroll
            for (int iq = 0; iq < SP_NQ; ++iq)
                seen[iq] = *reinterpret_cast<const volatile uint32_t *>(lds_bytes + SP_BND_OFF + (wave * SP_NQ + iq) * 256 + lane * 4);
            __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0)
            __builtin_amdgcn_s_barrier();
            if (bound_obj == cur && cur >= 0) {
#pragma unroll
                for (int iq = 0; iq < SP_NQ; ++iq)
                    if (valid[iq]) shared[iq] = __builtin_fmaxf(shared[iq], ord_dec(seen[iq]));
            }
        }
        // Between items nothing more is needed: every wave drained its own transfers (vmcnt(0)) and finished its LDS reads (the tiles of the last
        // chunk, its bound words: lgkmcnt(0)) before the barrier that ended the last step, so behind that barrier no transfer is in flight and no
        // wave reads the ring, the id / object slots or the bound words, and the next item's prologue may overwrite them.
    }
    if (aoc_lane() == 0) {
        atomicAdd(&g_prune_stats[0], (unsigned long long)n_seen * SP_NQ);
        atomicAdd(&g_prune_stats[1], (unsigned long long)n_rescored);
        atomicAdd(&g_prune_stats[2], (unsigned long long)n_any);
        atomicAdd(&g_prune_stats[3], (unsigned long long)n_seen);
        atomicAdd(&g_prune_stats[4], 0ull);      // reserved word, nothing added: compiles to the one load that the measured kernel ends with
    }
}

// ------------------------------------------------------------------------------------------
// Seeds of the shared bounds (round 6).  The pruning only bites once gbest[pixel][object] holds a good exact value, and until then almost every pair
// is rescored (at R = 1 a quarter of all pairs; profiles/r06_dense_experiments.txt, section 6).  A video's best match of query pixel i is, more often than
// not, the SAME pixel of the newest reference frame -- pool row n - m + i when the pool is whole frames of m rows.  This kernel evaluates that one pair per
// query pixel in plain fp32 and publishes  seed = 2^20 (q.r - |r|^2 / 2) - margin  for the object the row is labelled with, BEFORE the matrix kernel
// starts.  Whatever row that is, it is a real (pixel, kept row) pair of that object, and the margin keeps the seed at or below the value the matrix kernel
// itself computes for that pair, in the WORST case of every rounding: with M = 2^20 (|q||r| + |r|^2 / 2) >= every partial sum on either side,
//   the matrix kernel's 21 MFMAs round at most 21 x 16 times by half an ulp <= 2^-24 M each                          336 x 2^-24 M
//   this kernel's two fp32 dot products of C <= 100 terms (sequential adds) and the final subtraction                  ~210 x 2^-24 M
//   the ql.rl product the three-product value leaves out: <= 2^20 (2^-11 |q|)(2^-11 |r|)                              0.25 |q||r|
// margin = 4e-5 M + |q||r| + 16 (4e-5 > 546 x 2^-24 = 3.3e-5; tests/test_host_logic.py::test_dense_seed_margin_covers_the_worst_case replays the
// arithmetic in numpy).  Hence  seed <= exact(seed pair) <= exact(best pair) <= coarse(best pair) + eps : the best pair is still evaluated and the
// published maximum is the same number as without seeds -- the seeds only spare pairs that could never have held it.  (~5e-4 in squared-distance units
// on the bench's embeddings, below the kernel's own rescoring margin eps = 1.4e-3.)
constexpr int AOC_DENSE_SEED_FRAMES = 1;
__global__ __launch_bounds__(256) void dense_seed_kernel(const float *__restrict__ query, const float *__restrict__ q2, int64_t m, int C,
                                                          const float *__restrict__ pool, int64_t n, const uint32_t *__restrict__ right_bits, int n_obj,
                                                          const int32_t *__restrict__ gate, uint32_t *__restrict__ gbest) {
    if (*gate) return;
    // eight lanes per query pixel, a wave = eight consecutive pixels: their rows (and the candidate rows, consecutive as well) are read as whole 128-byte
    // lines; partial sums meet over three shuffles.  (One thread per pixel walked its two 400-byte rows alone: 37 us per launch on the frame's critical path.)
    const int sub = threadIdx.x & 7;
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
    const bool live = i < m;
    const int64_t ii = live ? i : m - 1;
    const uint32_t mask = (n_obj >= 32) ? 0xffffffffu : ((1u << n_obj) - 1u);
    const float4 *qr = reinterpret_cast<const float4 *>(query + (size_t)ii * C);
    const float qq = q2[ii];
    const int c4 = C >> 2;
    // the same pixel of the newest AOC_DENSE_SEED_FRAMES reference frames: where an object has moved over the pixel, the older frames seed another object
    for (int f = 0; f < AOC_DENSE_SEED_FRAMES && (int64_t)(f + 1) * m <= n; ++f) {
        const int64_t j = n - (int64_t)(f + 1) * m + ii;
        const uint32_t right = right_bits[j];
        const bool ok = live && (right & AOC_ROW_KEPT_BIT) && __popc(right & mask) == 1;      // (uniform over the pixel's eight lanes)
        const float4 *rr = reinterpret_cast<const float4 *>(pool + (size_t)j * C);
        float dot = 0.0f, r2 = 0.0f;
        for (int t = sub; t < c4; t += 8) {
            const float4 a = qr[t], b = rr[t];
            dot = dot + a.x * b.x; dot = dot + a.y * b.y; dot = dot + a.z * b.z; dot = dot + a.w * b.w;
            r2 = r2 + b.x * b.x; r2 = r2 + b.y * b.y; r2 = r2 + b.z * b.z; r2 = r2 + b.w * b.w;
        }
#pragma unroll
        for (int d = 1; d < 8; d <<= 1) {
            dot = dot + __shfl_xor(dot, d);
            r2 = r2 + __shfl_xor(r2, d);
        }
        if (ok && sub == 0) {
            const int o = __ffs((int)(right & mask)) - 1;
            const float value = 1048576.0f * (dot - 0.5f * r2);
            const float qr_n = sqrtf(qq * r2);
            const float seed = value - (4e-5f * (1048576.0f * (qr_n + 0.5f * r2)) + qr_n + 16.0f);
            atomicMax(gbest + (size_t)ii * n_obj + o, ord_enc(seed));
        }
    }
}

// out[i,o] = f( min(own_o, 5e4 + min_{o' != o} own_o') ), own_o = |q_i|^2 - 2^-19 max-accumulator (+inf: no pixel of o)
// (every word of gbest it reads is zeroed again: a caller that keeps the workspace across the frames of one pool state -- aoc_dense_match_min_split_cached
// -- starts the next frame without a memset)
__global__ __launch_bounds__(256) void dense_split_finalize_kernel(uint32_t *__restrict__ gbest, int64_t m, int n_obj,
                                                                    const int32_t *__restrict__ counts, const int32_t *__restrict__ gate,
                                                                    const float *__restrict__ q2, const float *__restrict__ obj_bias,
                                                                    float *__restrict__ out, int64_t pstride, int64_t ostride, int transform) {
    if (*gate) return;
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m) return;
    const float qq = q2[row];
    float own[16];
    int n_kept = 0;
#pragma unroll
    for (int o = 0; o < 16; ++o) {
        own[o] = INFINITY;
        if (o < n_obj && counts[o] > 0) {
            own[o] = qq + SP_UNSCALE * ord_dec(gbest[(size_t)row * n_obj + o]);
            gbest[(size_t)row * n_obj + o] = 0u;
            n_kept += counts[o];
        }
    }
#pragma unroll
    for (int o = 0; o < 16; ++o) {
        if (o < n_obj) {
            float others = INFINITY;
#pragma unroll
            for (int o2 = 0; o2 < 16; ++o2)
                if (o2 != o && o2 < n_obj) others = fminf(others, own[o2]);
            float v = fminf(own[o], others + AOC_PAD_DISTANCE);
            if (n_kept == 0) v = transform ? 1.0f : INFINITY;            // AEM:796-797
            else if (transform) v = aoc_proto_transform(v, obj_bias ? obj_bias[o] : 0.0f);
            out[row * pstride + o * ostride] = v;
        }
    }
}

// reused plan (aoc_dense_match_min_split_cached): the plan's gate already holds "a kept row is not one-hot | overflow at plan time"; the
// overflow word is sticky and may have been raised by a later query
__global__ void split_gate_refresh_kernel(const int32_t *__restrict__ overflow, int32_t *__restrict__ gate) {
    if (*overflow) atomicOr(gate, 1);
}

// The share of the stream's CUs that dense_prune_kernel's resident workgroups take, in 256ths (aoc_set_dense_share).  The rest of the CUs stays
// free for the kernels of other streams (the gates and the front end of the other sequence in flight) for the whole dense launch.
std::atomic<int> g_dense_share{AOC_DENSE_SHARE_DEFAULT};

struct SplitSizing {
    int splits, items, workgroups;
};
// budget: CUs the launching stream may use (0 = 256: no CU mask); share: 1 .. 256.
inline SplitSizing split_sizing(int64_t m, int budget, int share) {
    const int64_t row_blocks = (m + SP_ROWS_PER_BLOCK - 1) / SP_ROWS_PER_BLOCK;
    const int n_cu = budget > 0 ? budget : 256;
    // resident workgroups, one per CU: the share of the budget, a multiple of 8 from 8 up (the kernel's XCD map), at least one
    int64_t g = ((int64_t)n_cu * share) >> 8;
    if (g >= 8) g &= ~(int64_t)7;
    if (g < 1) g = 1;
    // The split count fills whole rounds of g.  Fewer splits share their bounds sooner (in-run launch 1.43 / 1.50 / 1.56 ms at 1 / 2 / 4 rounds of
    // the whole budget), more rounds leave a shorter ragged end.  At the whole budget (share 256) the rule is the one the one-workgroup-per-item
    // kernel was sized by, two rounds at most: the same splits as before.  A smaller g may take a third round, which keeps the splits near those of
    // the whole budget (51 row blocks on 224 CUs: 8 splits; on 136: 8 splits in three full rounds).
    const int max_rounds = share >= 256 ? 2 : 3;
    int best = 1;
    double best_eff = 0.0;
    for (int k = 1; k <= max_rounds; ++k) {
        int64_t ns = (g * k) / row_blocks;
        if (ns < 1) ns = 1;
        if (ns > 64) ns = 64;
        const int64_t blocks = row_blocks * ns;
        const int64_t rounds = (blocks + g - 1) / g;
        const double eff = (double)blocks / ((double)g * rounds);
        if (eff >= best_eff - 0.005) { best_eff = eff > best_eff ? eff : best_eff; best = (int)ns; }
    }
    const int64_t items = row_blocks * best;
    if (g > items) g = items;
    if (g >= 8) g &= ~(int64_t)7;
    return SplitSizing{best, (int)items, (int)g};
}

struct SplitWs {
    int32_t *gate, *n_tiles, *tile_rows, *tile_obj;
    uint32_t *pmax, *gbest;
    void *fp32_ws;
    size_t fp32_bytes, total;
    int64_t tile_capacity;
};
inline SplitWs split_carve(void *base, int64_t m, int64_t n, int n_obj) {
    SplitWs w;
    char *p = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *r = p ? p + off : nullptr; off += aoc_align_up(bytes, 256); return r; };
    w.tile_capacity = (n + SP_TILE - 1) / SP_TILE + n_obj + SP_TILE_SLACK;
    w.gate = reinterpret_cast<int32_t *>(take(16));
    w.n_tiles = w.gate ? w.gate + 2 : nullptr;
    w.pmax = w.gate ? reinterpret_cast<uint32_t *>(w.gate + 3) : nullptr;
    w.tile_rows = reinterpret_cast<int32_t *>(take((size_t)w.tile_capacity * SP_TILE * sizeof(int32_t)));
    w.tile_obj = reinterpret_cast<int32_t *>(take((size_t)w.tile_capacity * sizeof(int32_t)));
    w.gbest = reinterpret_cast<uint32_t *>(take((size_t)m * n_obj * sizeof(uint32_t)));
    w.fp32_bytes = aoc_dense_match_workspace_bytes(m, n, n_obj);
    w.fp32_ws = take(w.fp32_bytes);
    w.total = off;
    return w;
}

}  // namespace

extern "C" {

size_t aoc_split_record_bytes(int C) { return (C >= 4 && (C & 3) == 0 && C <= SP_NORM_SLOT) ? (size_t)SP_REC * 16 : 0; }

int aoc_split_rows(const float *x, int64_t n, int C, void *records, float *sqnorm, int32_t *overflow_flag, aoc_stream_t stream) {
    if (!x || !records || !overflow_flag || n < 0) return AOC_ERR_INVALID_ARG;
    if (aoc_off16(x, records)) return AOC_ERR_INVALID_ARG;                 // float4 loads of the rows, uint4 stores of the records
    if (aoc_split_record_bytes(C) == 0) return AOC_ERR_UNSUPPORTED;
    if (n == 0) return AOC_OK;
    const int64_t total = n * SP_KS;
    hipLaunchKernelGGL(split_rows_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, aoc_hip_stream(stream), x, n, C,
                       static_cast<uint4 *>(records), sqnorm, overflow_flag);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

size_t aoc_split_rows_tiled_bytes(int64_t n, int C) {
    if (n < 0 || aoc_split_record_bytes(C) == 0) return 0;
    return (size_t)((n + 31) / 32) * 32 * SP_REC * 16;
}

int aoc_split_rows_tiled(const float *x, int64_t n, int C, void *records, float *sqnorm, int32_t *overflow_flag, aoc_stream_t stream) {
    if (!x || !records || !overflow_flag || n < 0) return AOC_ERR_INVALID_ARG;
    if (aoc_off16(x, records)) return AOC_ERR_INVALID_ARG;                 // float4 loads of the rows, uint4 stores of the records
    if (aoc_split_record_bytes(C) == 0) return AOC_ERR_UNSUPPORTED;
    if (n == 0) return AOC_OK;
    const int64_t total = (n + 31) / 32 * 32 * SP_KS;
    hipLaunchKernelGGL(split_rows_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, aoc_hip_stream(stream), x, n, C,
                       static_cast<uint4 *>(records), sqnorm, overflow_flag);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

size_t aoc_dense_match_split_workspace_bytes(int64_t m, int64_t n, int n_obj) {
    if (m < 1 || n < 1 || n_obj < 1) return 0;
    return split_carve(nullptr, m, n, n_obj).total;
}

int aoc_dense_match_min_split(const float *query, const void *query_rec, const float *query_sqnorm, int query_rec_tiled, int64_t m, int C, const float *pool,
                              const void *pool_rec, const int32_t *overflow_flag, int64_t n, const uint32_t *right_bits,
                              const uint32_t *wrong_bits, const int32_t *fg_rows, const int32_t *obj_rows, const int32_t *counts,
                              const int32_t *obj_offsets, const float *obj_bias, int n_obj, float *out, int64_t out_pixel_stride,
                              int64_t out_obj_stride, int transform, void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    return aoc_dense_match_min_split_cached(query, query_rec, query_sqnorm, query_rec_tiled, m, C, pool, pool_rec, overflow_flag, n, right_bits, wrong_bits,
                                            fg_rows, obj_rows, counts, obj_offsets, obj_bias, n_obj, out, out_pixel_stride, out_obj_stride, transform, workspace,
                                            workspace_bytes, 0, stream);
}

int aoc_dense_match_min_split_cached(const float *query, const void *query_rec, const float *query_sqnorm, int query_rec_tiled, int64_t m, int C, const float *pool,
                                     const void *pool_rec, const int32_t *overflow_flag, int64_t n, const uint32_t *right_bits,
                                     const uint32_t *wrong_bits, const int32_t *fg_rows, const int32_t *obj_rows, const int32_t *counts,
                                     const int32_t *obj_offsets, const float *obj_bias, int n_obj, float *out, int64_t out_pixel_stride,
                                     int64_t out_obj_stride, int transform, void *workspace, size_t workspace_bytes, int reuse_plan, aoc_stream_t stream) {
    if (!query || !query_rec || !query_sqnorm || !pool || !pool_rec || !overflow_flag || !right_bits || !wrong_bits || !fg_rows ||
        !obj_rows || !counts || !obj_offsets || !out || !workspace)
        return AOC_ERR_INVALID_ARG;
    // float4 rows in the seed and the exact-fp32 kernels, uint4 / LDS-direct records, LDS-direct tile lists out of the workspace
    if (aoc_off16(query, query_rec, pool, pool_rec, workspace)) return AOC_ERR_INVALID_ARG;
    if (m < 1 || n < 1 || n >= (1ll << 31) - 4096 || n_obj < 1) return AOC_ERR_INVALID_ARG;
    if (aoc_split_record_bytes(C) == 0 || n_obj > 16) return AOC_ERR_UNSUPPORTED;
    if (workspace_bytes < aoc_dense_match_split_workspace_bytes(m, n, n_obj)) return AOC_ERR_WORKSPACE;
    hipStream_t st = aoc_hip_stream(stream);
    const SplitWs w = split_carve(workspace, m, n, n_obj);
    if (reuse_plan) {
        // same pool rows, labels and records as the call that built the plan in this workspace: tile lists, norm maxima and the one-hot check
        // stand; gbest was left clean by that call's finalize kernel
        hipLaunchKernelGGL(split_gate_refresh_kernel, dim3(1), dim3(1), 0, st, overflow_flag, w.gate);
    } else {
        if (hipMemsetAsync(w.gate, 0, 16, st) != hipSuccess) return AOC_ERR_LAUNCH;
        if (hipMemsetAsync(w.gbest, 0, (size_t)m * n_obj * sizeof(uint32_t), st) != hipSuccess) return AOC_ERR_LAUNCH;
        const int64_t plan_threads = w.tile_capacity * SP_TILE > n ? w.tile_capacity * SP_TILE : n;
        hipLaunchKernelGGL(split_plan_kernel, dim3((unsigned)((plan_threads + 255) / 256)), dim3(256), 0, st, obj_rows, counts, obj_offsets, n_obj, n,
                           right_bits, wrong_bits, overflow_flag, static_cast<const uint4 *>(pool_rec), w.tile_capacity, w.tile_rows, w.tile_obj,
                           w.n_tiles, w.gate, w.pmax);
    }
    if (n >= m)
        hipLaunchKernelGGL(dense_seed_kernel, dim3((unsigned)((m * 8 + 255) / 256)), dim3(256), 0, st, query, query_sqnorm, m, C, pool, n, right_bits, n_obj, w.gate,
                           w.gbest);
    const SplitSizing sz = split_sizing(m, aoc_stream_cus(), g_dense_share.load(std::memory_order_relaxed));
    const dim3 grid((unsigned)sz.workgroups);
    const AocDenseProbe probe = aoc_take_dense_probe();
    static const bool lds_ok = hipFuncSetAttribute(reinterpret_cast<const void *>(dense_prune_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   SP_LDS_BYTES) == hipSuccess;
    if (!lds_ok) return AOC_ERR_LAUNCH;
    if (probe.start) (void)hipEventRecord(probe.start, st);
    hipLaunchKernelGGL(dense_prune_kernel<0>, grid, dim3(SP_NW * 64), SP_LDS_BYTES, st, static_cast<const uint4 *>(query_rec), query_sqnorm, m,
                       static_cast<const uint4 *>(pool_rec), w.tile_rows, w.tile_obj, w.n_tiles, w.gate, w.pmax, n_obj, w.gbest, query_rec_tiled ? 1 : 0,
                       sz.splits);
    if (probe.stop) (void)hipEventRecord(probe.stop, st);
    hipLaunchKernelGGL(dense_split_finalize_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, w.gbest, m, n_obj, counts, w.gate,
                       query_sqnorm, obj_bias, out, out_pixel_stride, out_obj_stride, transform);
    AOC_RETURN_IF_LAUNCH_FAILED();
    // exact-fp32 kernels: run only when the gate is set
    return aoc_dense_match_min_gated(query, m, C, pool, fg_rows, counts + n_obj, n, wrong_bits, obj_bias, n_obj, out, out_pixel_stride,
                                     out_obj_stride, transform, w.fp32_ws, w.fp32_bytes, w.gate, stream);
}

static std::atomic<int> g_stream_cus{0};
int aoc_set_stream_cus(int n_cus) {
    if (n_cus < 0) return AOC_ERR_INVALID_ARG;
    g_stream_cus.store(n_cus, std::memory_order_relaxed);
    return AOC_OK;
}

int aoc_set_dense_share(int share_256) {
    if (share_256 < 1 || share_256 > 256) return AOC_ERR_INVALID_ARG;
    g_dense_share.store(share_256, std::memory_order_relaxed);
    return AOC_OK;
}
int aoc_dense_share(void) { return g_dense_share.load(std::memory_order_relaxed); }

int aoc_dense_split_sizing(int64_t m, int budget, int share_256, int32_t *splits, int32_t *items, int32_t *workgroups) {
    if (m < 1 || m >= (1ll << 31) || budget < 0 || share_256 < 1 || share_256 > 256 || !splits || !items || !workgroups) return AOC_ERR_INVALID_ARG;
    const SplitSizing sz = split_sizing(m, budget, share_256);
    *splits = sz.splits;
    *items = sz.items;
    *workgroups = sz.workgroups;
    return AOC_OK;
}

// Developer counters of the coarse-then-rescore kernel, summed over all launches since the last reset:
// out[0] (reference tile, query tile) pairs tested, out[1] pairs rescored, out[2] reference tiles with a rescoring, out[3] reference tiles.
int aoc_dense_prune_stats(uint64_t *out4, int reset) {
    if (!out4) return AOC_ERR_INVALID_ARG;
    uint64_t v[8];
    const int rc = aoc_dense_prune_stats_ex(v, reset);
    for (int i = 0; i < 4 && rc == AOC_OK; ++i) out4[i] = v[i];
    return rc;
}

// out8[0..3] as aoc_dense_prune_stats; out8[4..7] reserved (0).
int aoc_dense_prune_stats_ex(uint64_t *out8, int reset) {
    if (!out8) return AOC_ERR_INVALID_ARG;
    unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_prune_stats), sizeof(v)) != hipSuccess) return AOC_ERR_LAUNCH;
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    if (reset) {
        const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_prune_stats), z, sizeof(z)) != hipSuccess) return AOC_ERR_LAUNCH;
    }
    return AOC_OK;
}

}  // extern "C"

// the budget of the call in progress on this thread (aoc_frame_enqueue: aoc_frame_desc.stream_cus), else the process-wide setting
static thread_local int t_stream_cus = 0;
int aoc_stream_cus() { return t_stream_cus > 0 ? t_stream_cus : g_stream_cus.load(std::memory_order_relaxed); }
int aoc_stream_cus_scope(int n_cus) {
    const int before = t_stream_cus;
    t_stream_cus = n_cus > 0 ? n_cus : 0;
    return before;
}
