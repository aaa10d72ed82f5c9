// Pileup on gfx950: per genome position, what the mapped reads say there, and the consensus call.
//
// An alignment is (pos, read, ops): ops one byte per column as chiron_align_trace codes them (0 '=', 1 'X', 2 'I', 3 'D'), pos the
// genome position of its first reference base.  For column j let q be the reference-consuming columns ('=', 'X', 'D') before it
// and i the read-consuming ones ('=', 'X', 'I').  With S = CHIRON_PILEUP_INS_SLOTS, per position g:
//   base[g][c]    '=' / 'X' columns at g = pos + q whose read base read[i] is c (0..4; the column's letter is not looked at)
//   del[g]        'D' columns at g
//   ins[g][k][c]  'I' columns whose reference-consuming predecessor sits at g = pos + q - 1, k 'I' columns after it, k < S
//   over[g]       the 'I' columns with k == S: one per alignment whose insertion after g is longer than S
// An 'I' column with q = 0 or q = m (m the alignment's reference-consuming columns) is clipping: counted nowhere per position.
// The call per position is integer arithmetic on those counts.                     (include/chiron_amd.h)
//
// pileup_count_kernel: one workgroup of 256 threads per alignment, alignment p on workgroup p mod the group count.  Columns are
// taken in chunks of 256 x PER: thread t owns columns base + s * 256 + t, s = 0 .. PER-1, so the 64 lanes of a wave hold 64
// consecutive columns and their adds land on runs of consecutive addresses within a few planes (the count planes are planar:
// [plane][position]).  q, i and k need two exclusive sums (the 'I' and the 'D' columns before j; both fit 16 bits within 256
// columns and share one 32-bit scan) and one running maximum (the last column before j that is not an 'I'): within a wave by
// cross-lane shuffles, across the four waves through eight LDS words, from sub-chunk to sub-chunk in three registers that every
// thread keeps alike.  One barrier per 256 columns (the LDS words are double-buffered).  Counts are added with relaxed
// agent-scope int32 atomic adds without a return value: integer sums do not depend on the order, so the result is exact and
// reproducible, and an alignment's contribution depends on nothing but that alignment.  Every offset is 64-bit.
//
// pileup_call_kernel: one thread per position; reads the planes (coalesced across the wave) and the reference code, applies the
// rule, writes depth and one 8-byte record.  No float arithmetic anywhere.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/chiron_amd.h"
#include "align_common.h"

namespace chiron {

namespace {

constexpr int NT = CHIRON_PILEUP_THREADS;
constexpr int PER = 4;                        // sub-chunks of NT columns whose op bytes are loaded ahead of their scans
constexpr int S = CHIRON_PILEUP_INS_SLOTS;
constexpr int PLANES = CHIRON_PILEUP_PLANES;
constexpr int PLANE_DEL = 5, PLANE_INS = 6, PLANE_OVER = PLANES - 1;
constexpr int MAX_GROUPS = 2048;              // workgroups of one launch
static_assert(NT == 256, "the cross-wave step below is written for four waves of 64");

struct PileupAln {
  int64_t read;              // the read's first code in `codes`
  int64_t ops;               // its first column in `ops`
  int64_t rel;               // pos - g0
  int32_t ncols;             // 0: the alignment touches no position of the tile (the host decided), nothing to do
  int32_t m;                 // its reference-consuming columns
};
struct PileupParams {
  const uint8_t* codes;
  const uint8_t* ops;
  const PileupAln* aln;      // [alignments]
  int64_t alignments;
  int64_t tile;              // positions of the tile, g1 - g0
  int32_t* counts;           // [PLANES][tile]
};
struct PileupLayout {
  size_t aln, codes, ops, ref, counts, depth, call, bytes;
};

__device__ __forceinline__ void add_one(int32_t* p) {
  (void)__hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CHIRON_PILEUP_THREADS) void pileup_count_kernel(PileupParams p) {
  __shared__ int wave_sum[2][4];
  __shared__ int wave_last[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tile = p.tile;
  int par = 0;               // which half of the LDS words this scan uses; alike in every thread
  for (int64_t a = blockIdx.x; a < p.alignments; a += gridDim.x) {
    const PileupAln r = p.aln[a];
    const int ncols = r.ncols, m = r.m;
    const uint8_t* __restrict__ ops = p.ops + r.ops;
    const uint8_t* __restrict__ read = p.codes + r.read;
    int nI = 0, nD = 0, last = -1;      // 'I' and 'D' columns before the sub-chunk, the last column before it that is no 'I'
    for (int base = 0; base < ncols; base += NT * PER) {
      // q at the chunk's first column is base - nI; once even an insertion's anchor, pos + q - 1, lies past the tile, so does
      // everything after it
      if (r.rel + (int64_t)(base - nI) - 1 >= tile) break;
      unsigned op[PER];
#pragma unroll
      for (int s = 0; s < PER; ++s) {
        const int j = base + s * NT + tid;
        op[s] = j < ncols ? (unsigned)ops[j] : 4u;       // 4: no column
      }
#pragma unroll
      for (int s = 0; s < PER; ++s) {
        const int j = base + s * NT + tid;
        const unsigned o = op[s];
        const int own = (o == 2u ? 1 : 0) | (o == 3u ? 1 << 16 : 0);
        int v = own;                                     // inclusive sums of the wave: 'I' columns low, 'D' columns high
        int l = (o != 2u && o != 4u) ? j : -1;           // inclusive maximum: the last column up to j that is no 'I'
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int tv = __shfl_up(v, d);
          const int tl = __shfl_up(l, d);
          if (lane >= d) {
            v += tv;
            l = tl > l ? tl : l;
          }
        }
        if (lane == 63) {
          wave_sum[par][wave] = v;
          wave_last[par][wave] = l;
        }
        __syncthreads();
        int pre = 0, tot = 0, pl = -1, tl = -1;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int sv = wave_sum[par][w], lv = wave_last[par][w];
          if (w < wave) {
            pre += sv;
            pl = lv > pl ? lv : pl;
          }
          tot += sv;
          tl = lv > tl ? lv : tl;
        }
        par ^= 1;            // the next scan writes the other half: a thread still reading this one is not overtaken
        if (o != 4u) {
          const int before = v + pre - own;              // exclusive
          const int q = j - (nI + (before & 0xffff));
          const int i = j - (nD + (before >> 16));
          if (o < 2u) {
            const int64_t g = r.rel + q;
            if (g >= 0 && g < tile) add_one(p.counts + (int64_t)read[i] * tile + g);
          } else if (o == 3u) {
            const int64_t g = r.rel + q;
            if (g >= 0 && g < tile) add_one(p.counts + (int64_t)PLANE_DEL * tile + g);
          } else if (q != 0 && q != m) {
            const int64_t g = r.rel + q - 1;
            if (g >= 0 && g < tile) {
              int lb = l > pl ? l : pl;                  // an 'I' column's own entry is -1: inclusive is exclusive here
              lb = last > lb ? last : lb;
              const int k = j - lb - 1;
              if (k < S)
                add_one(p.counts + (int64_t)(PLANE_INS + 5 * k + read[i]) * tile + g);
              else if (k == S)
                add_one(p.counts + (int64_t)PLANE_OVER * tile + g);
            }
          }
        }
        nI += tot & 0xffff;
        nD += tot >> 16;
        last = tl > last ? tl : last;
      }
    }
  }
}

__global__ __launch_bounds__(CHIRON_PILEUP_THREADS) void pileup_call_kernel(const int32_t* __restrict__ counts, const uint8_t* __restrict__ ref,
                                                                              int64_t tile, int32_t min_depth, int32_t* __restrict__ depth_out,
                                                                              unsigned long long* __restrict__ call_out) {
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (g >= tile) return;
  const int r = ref[g];
  const int b0 = counts[g], b1 = counts[tile + g], b2 = counts[2 * tile + g], b3 = counts[3 * tile + g];
  const int del = counts[(int64_t)PLANE_DEL * tile + g];
  const int depth = b0 + b1 + b2 + b3 + counts[4 * tile + g] + del;
  depth_out[g] = depth;
  unsigned long long rec;
  if (depth < min_depth) {
    rec = (unsigned long long)r | (1ull << 48);
  } else {
    // key (count, c == r, -c): ascending c, a later base replaces the best only with a larger count, or an equal one when it is r
    int best = b0, code = 0;
    if (b1 > best || (b1 == best && r == 1)) { best = b1; code = 1; }
    if (b2 > best || (b2 == best && r == 2)) { best = b2; code = 2; }
    if (b3 > best || (b3 == best && r == 3)) { best = b3; code = 3; }
    if (del > best) code = 5;
    else if (best == 0) code = r;
    rec = (unsigned long long)code;
    unsigned long long n = 0;
    bool open = true;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const int32_t* pl = counts + (int64_t)(PLANE_INS + 5 * k) * tile + g;
      const int i0 = pl[0], i1 = pl[tile], i2 = pl[2 * tile], i3 = pl[3 * tile], i4 = pl[4 * tile];
      open = open && 2 * (int64_t)(i0 + i1 + i2 + i3 + i4) > (int64_t)depth;
      if (open) {
        int bi = i0, ci = 0;
        if (i1 > bi) { bi = i1; ci = 1; }
        if (i2 > bi) { bi = i2; ci = 2; }
        if (i3 > bi) { bi = i3; ci = 3; }
        if (bi == 0) ci = 4;
        rec |= (unsigned long long)ci << (16 + 8 * k);
        ++n;
      }
    }
    rec |= n << 8;
  }
  call_out[g] = rec;         // bytes 0..7, little-endian: code, inserted bases, their four codes, status, 0
}

chiron_status pileup_layout(int64_t alignments, int64_t read_bytes, int64_t column_bytes, int64_t tile, PileupLayout* l) {
  if (alignments < 0 || read_bytes < 0 || column_bytes < 0 || tile < 0)
    return set_error(CHIRON_ERR_INVALID, "pileup: negative alignments / read_bytes / column_bytes / tile_len");
  if (alignments > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "pileup: %lld alignments in one call, at most 2^24", (long long)alignments);
  if (tile > CHIRON_PILEUP_MAX_TILE)
    return set_error(CHIRON_ERR_OVERFLOW, "pileup: a tile of %lld positions, at most %d", (long long)tile, CHIRON_PILEUP_MAX_TILE);
  // an alignment has at most CHIRON_PILEUP_MAX_COLUMNS columns and as many read bases
  if (read_bytes > MAX_BATCH_ITEMS * CHIRON_PILEUP_MAX_COLUMNS || column_bytes > MAX_BATCH_ITEMS * CHIRON_PILEUP_MAX_COLUMNS)
    return set_error(CHIRON_ERR_OVERFLOW, "pileup: %lld read bytes / %lld column bytes, at most 2^48 each", (long long)read_bytes, (long long)column_bytes);
  l->aln = 0;
  l->codes = l->aln + up256((size_t)alignments * sizeof(PileupAln));
  l->ops = l->codes + up256((size_t)read_bytes);
  l->ref = l->ops + up256((size_t)column_bytes);
  l->counts = l->ref + up256((size_t)tile);
  l->depth = l->counts + up256((size_t)PLANES * (size_t)tile * sizeof(int32_t));
  l->call = l->depth + up256((size_t)tile * sizeof(int32_t));
  l->bytes = l->call + up256((size_t)tile * 8);
  return CHIRON_OK;
}

}  // namespace
}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_pileup_workspace_size(int64_t alignments, int64_t read_bytes, int64_t column_bytes, int64_t tile_len, size_t* bytes) {
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "chiron_pileup_workspace_size: null bytes");
  PileupLayout l;
  chiron_status st = pileup_layout(alignments, read_bytes, column_bytes, tile_len, &l);
  if (st) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_pileup(int32_t device_id, const uint8_t* codes, const int64_t* read_off, const uint8_t* ops, const int64_t* ops_off,
                                       const int64_t* pos, int64_t alignments, int64_t g0, int64_t g1, const uint8_t* ref_codes, int32_t min_depth,
                                       uint32_t flags, int32_t* counts_out, int32_t* depth_out, uint8_t* call_out, int64_t* clipped_out,
                                       void* workspace, void* stream_) {
  if (alignments < 0) return set_error(CHIRON_ERR_INVALID, "chiron_pileup: alignments %lld", (long long)alignments);
  if (flags) return set_error(CHIRON_ERR_INVALID, "chiron_pileup: unknown flags 0x%x", flags);
  if (g0 < 0 || g1 < g0) return set_error(CHIRON_ERR_INVALID, "chiron_pileup: tile [%lld, %lld)", (long long)g0, (long long)g1);
  if (min_depth < 0) return set_error(CHIRON_ERR_INVALID, "chiron_pileup: min_depth %d", min_depth);
  if (alignments > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "chiron_pileup: %lld alignments in one call, at most 2^24", (long long)alignments);
  const int64_t tile = g1 - g0;
  if (tile > CHIRON_PILEUP_MAX_TILE)
    return set_error(CHIRON_ERR_OVERFLOW, "chiron_pileup: a tile of %lld positions, at most %d", (long long)tile, CHIRON_PILEUP_MAX_TILE);
  if (!clipped_out) return set_error(CHIRON_ERR_INVALID, "chiron_pileup: null clipped_out");
  if (alignments > 0 && (!read_off || !ops_off || !pos)) return set_error(CHIRON_ERR_INVALID, "chiron_pileup: null operand");
  if (tile > 0 && (!ref_codes || !depth_out || !call_out)) return set_error(CHIRON_ERR_INVALID, "chiron_pileup: null ref_codes / depth_out / call_out");
  // offsets first (they bound what may be read of `codes` and `ops`), then every column and every code
  if (alignments > 0) {
    int64_t longest = 0, sum = 0;   // not needed here: the sizes below come from the offsets' ends
    chiron_status st = check_offsets("chiron_pileup", "read", "alignment", "read bases", read_off, alignments, CHIRON_PILEUP_MAX_COLUMNS, &longest, &sum);
    if (!st) st = check_offsets("chiron_pileup", "ops", "alignment", "columns", ops_off, alignments, CHIRON_PILEUP_MAX_COLUMNS, &longest, &sum);
    if (st) return st;
  }
  const int64_t read_lo = alignments ? read_off[0] : 0, ops_lo = alignments ? ops_off[0] : 0;
  const int64_t read_bytes = alignments ? read_off[alignments] - read_lo : 0, column_bytes = alignments ? ops_off[alignments] - ops_lo : 0;
  if (read_bytes > 0 && !codes) return set_error(CHIRON_ERR_INVALID, "chiron_pileup: null codes");
  if (column_bytes > 0 && !ops) return set_error(CHIRON_ERR_INVALID, "chiron_pileup: null ops");
  std::vector<PileupAln> recs((size_t)alignments);
  int64_t clipped = 0;
  for (int64_t a = 0; a < alignments; ++a) {
    const int64_t n = read_off[a + 1] - read_off[a], cols = ops_off[a + 1] - ops_off[a];
    const uint8_t* o = ops + ops_off[a];
    int64_t cnt[4] = {0, 0, 0, 0}, lead = 0, trail = 0;
    for (int64_t j = 0; j < cols; ++j) {
      if (o[j] > 3) return set_error(CHIRON_ERR_INVALID, "chiron_pileup: op %d at column %lld of alignment %lld outside 0..3", (int)o[j], (long long)j, (long long)a);
      ++cnt[o[j]];
      trail = o[j] == 2 ? trail + 1 : 0;
      if (lead == j && o[j] == 2) ++lead;
    }
    if (cnt[0] + cnt[1] + cnt[2] != n)
      return set_error(CHIRON_ERR_INVALID, "chiron_pileup: the columns of alignment %lld consume %lld read bases, its read has %lld", (long long)a,
                       (long long)(cnt[0] + cnt[1] + cnt[2]), (long long)n);
    const uint8_t* c = codes + read_off[a];
    for (int64_t i = 0; i < n; ++i)
      if (c[i] > 4)
        return set_error(CHIRON_ERR_INVALID, "chiron_pileup: code %d at %lld of read %lld outside 0..4", (int)c[i], (long long)i, (long long)a);
    const int64_t m = cnt[0] + cnt[1] + cnt[3];
    clipped += m == 0 ? cols : lead + trail;          // without a reference base, q = 0 = m for every column
    PileupAln& r = recs[(size_t)a];
    r.read = read_off[a] - read_lo;
    r.ops = ops_off[a] - ops_lo;
    r.m = (int32_t)m;
    // its positions are pos .. pos + m - 1: outside [g0, g1) it has nothing to count (and pos - g0 might not even be representable)
    const bool touches = m > 0 && pos[a] < g1 && pos[a] > g0 - m;
    r.rel = touches ? pos[a] - g0 : 0;
    r.ncols = touches ? (int32_t)cols : 0;
  }
  *clipped_out = clipped;
  if (tile == 0) return CHIRON_OK;
  for (int64_t g = 0; g < tile; ++g)
    if (ref_codes[g] > 4) return set_error(CHIRON_ERR_INVALID, "chiron_pileup: reference code %d at tile position %lld outside 0..4", (int)ref_codes[g], (long long)g);
  PileupLayout l;
  chiron_status st = pileup_layout(alignments, read_bytes, column_bytes, tile, &l);
  if (st) return st;
  if ((st = use_device_workspace("chiron_pileup", device_id, workspace))) return st;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  const size_t count_bytes = (size_t)PLANES * (size_t)tile * sizeof(int32_t);
  if ((alignments > 0 && hipMemcpyAsync(ws + l.aln, recs.data(), recs.size() * sizeof(PileupAln), hipMemcpyHostToDevice, stream) != hipSuccess) ||
      (read_bytes > 0 && hipMemcpyAsync(ws + l.codes, codes + read_lo, (size_t)read_bytes, hipMemcpyHostToDevice, stream) != hipSuccess) ||
      (column_bytes > 0 && hipMemcpyAsync(ws + l.ops, ops + ops_lo, (size_t)column_bytes, hipMemcpyHostToDevice, stream) != hipSuccess) ||
      hipMemcpyAsync(ws + l.ref, ref_codes, (size_t)tile, hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemsetAsync(ws + l.counts, 0, count_bytes, stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "chiron_pileup: copying the alignments to the device failed");
  if (alignments > 0) {
    PileupParams p;
    p.codes = (const uint8_t*)(ws + l.codes);
    p.ops = (const uint8_t*)(ws + l.ops);
    p.aln = (const PileupAln*)(ws + l.aln);
    p.alignments = alignments;
    p.tile = tile;
    p.counts = (int32_t*)(ws + l.counts);
    const int groups = (int)(alignments < MAX_GROUPS ? alignments : MAX_GROUPS);
    hipLaunchKernelGGL(pileup_count_kernel, dim3(groups), dim3(NT), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return set_error(CHIRON_ERR_DEVICE, "chiron_pileup: launching the count kernel failed");
  }
  hipLaunchKernelGGL(pileup_call_kernel, dim3((unsigned)((tile + NT - 1) / NT)), dim3(NT), 0, stream, (const int32_t*)(ws + l.counts),
                     (const uint8_t*)(ws + l.ref), tile, min_depth, (int32_t*)(ws + l.depth), (unsigned long long*)(ws + l.call));
  if (hipGetLastError() != hipSuccess) return set_error(CHIRON_ERR_DEVICE, "chiron_pileup: launching the call kernel failed");
  if ((counts_out && hipMemcpyAsync(counts_out, ws + l.counts, count_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
      hipMemcpyAsync(depth_out, ws + l.depth, (size_t)tile * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(call_out, ws + l.call, (size_t)tile * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return set_error(CHIRON_ERR_DEVICE, "chiron_pileup: the pileup kernels failed (%s)", hipGetErrorString(hipGetLastError()));
  return CHIRON_OK;
}
