// Seeding of the read mapper on gfx950: k-mer lookup, diagonal votes and the candidate of every read, equal to map.vote
// (chiron_amd/map.py) field for field.
//
//   k = 15, 2 bits a base, first base highest.  Each read is scored as given (strand 0) and reverse-complemented (strand 1); a
//   k-mer that holds a code above 3 is skipped.  A hit of read position r at genome position g votes for delta = g - r, in bin
//   floor(delta / 256).  The score of a bin that holds a hit is its count plus the next bin's; the best score wins, ties to
//   strand 0, then to the smaller bin.  votes_second is the other strand's best, or the best score of a bin of the winning strand
//   more than n / 256 + 2 bins from the winner.  The candidate is the hit of rank (votes - 1) / 2 among the hits of the winning
//   two bins, ordered by (delta, g).                                                                     (include/chiron_amd.h)
//
// Work mapping: one workgroup of 256 threads per read, read q on workgroup q mod the group count.  The workgroup owns two rows
// of the workspace: per strand, (first index entry, count) of every k-mer position, so that the lookup runs once and the later
// passes replay the hits from it, and a dense int32 histogram of the bins.  Nothing is sorted and the dense histogram is never
// scanned; every pass walks the hits:
//   1 lookup   thread t rolls the k-mers of a contiguous chunk of read positions, forward and reverse-complement value at once
//              (the k-mer at p is strand 0's position p and, complemented, strand 1's position n - 15 - p), searches the sorted
//              index (lower bound, then a gallop to the end of the run), stores (first, count) and adds 1 to the bin of each hit.
//   2 winner   score(b) = cnt[b] + cnt[b + 1] of each hit's bin; a block maximum of (score, -bin) per strand.
//   3 far, delta  over the winning strand: the far maximum, and a 512-counter histogram in LDS of delta over the winning two
//              bins; a prefix sum finds the delta that holds rank (votes - 1) / 2 and the rank j left within it.
//   4 rank     hits of one delta are ordered by g = delta + r, and a read position hits distinct genome positions, so each r
//              holds at most one: counts per 256 positions, a prefix sum, then flags of the 256 positions of that block and a
//              prefix sum give the j-th.
//   5 clear    the hits once more, storing zeros, before the workgroup takes its next read.
// Integer sums do not depend on the order the atomic adds land in, and nothing else does: the maxima are over total orders and
// the ranks come from counts.  A rank no counter covers means a counter was stale; the read then reports -1 votes and the call
// fails with CHIRON_ERR_STATE rather than return a wrong candidate.
//
// Memory order: the histogram is written by device-scope atomic adds, which execute in L2, and read back by other threads of
// the workgroup, so the reads are device-scope relaxed loads (they bypass the CU's vector cache) and every phase ends with a
// device-scope fence and a barrier.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/chiron_amd.h"
#include "align_common.h"

namespace chiron {

namespace {

constexpr int NT = CHIRON_SEED_THREADS;
constexpr int K = CHIRON_SEED_K;
constexpr int SHIFT = 8;                         // log2(CHIRON_SEED_BIN)
constexpr int SPAN = 2 * CHIRON_SEED_BIN;        // deltas of the winning two bins
static_assert(CHIRON_SEED_BIN == 1 << SHIFT && SPAN == 2 * NT, "rank_find covers two counters a thread");
static_assert(CHIRON_INFIX_MAX_READ / NT <= SPAN, "one counter per 256 read positions fits the same array");

struct SeedRead {
  int64_t start;   // of the read in the packed codes
  int32_t n, pad;
};

struct SeedParams {
  const uint32_t* idx_val;
  const int32_t* idx_pos;
  int32_t n_index;
  const uint8_t* codes;
  const SeedRead* read;
  int64_t reads;
  int2* kc;          // [groups][2][kc_stride]: (first index entry, count) of the k-mer at each read position, per strand
  int64_t kc_stride;
  int32_t* hist;     // [groups][2][nbins], zero between reads
  int64_t nbins;
  int32_t off;       // a multiple of 256 at or above the longest read: bin index = (delta + off) >> 8
  int32_t* out;      // [reads][5]: votes, votes_second, strand, delta, g
};

__device__ __forceinline__ void phase_sync() {
  __threadfence();
  __syncthreads();
}
__device__ __forceinline__ int32_t counter(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void counter_clear(int32_t* p) { __hip_atomic_store(p, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (first entry, count) of the run of v in the sorted val[0 .. n)
__device__ inline int2 lookup(const uint32_t* __restrict__ val, int32_t n, uint32_t v) {
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (val[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo >= n || val[lo] != v) return make_int2(lo, 0);
  int64_t e = 1;
  while (lo + e < n && val[lo + e] == v) e <<= 1;       // val[lo + e / 2] is v; val[lo + e] is not, or lies past the end
  int64_t a = lo + (e >> 1) + 1, b = lo + e < n ? lo + e : n;
  while (a < b) {
    const int64_t mid = a + ((b - a) >> 1);
    if (val[mid] == v)
      a = mid + 1;
    else
      b = mid;
  }
  return make_int2(lo, (int32_t)(a - lo));
}

// h[0 .. 512) in LDS, complete and synchronised: the i with sum(h[0 .. i)) <= rank < sum(h[0 .. i]) and what is left of the
// rank within it; i = -1 when the counters do not reach the rank.  Leaves the arrays free for the next use.
__device__ inline void rank_find(const int32_t* h, int32_t* scan, int32_t* res, int32_t rank, int32_t* idx, int32_t* rem) {
  const int tid = threadIdx.x;
  const int32_t a = h[2 * tid], b = h[2 * tid + 1];
  scan[tid] = a + b;
  if (tid == 0) res[0] = -1, res[1] = 0;
  __syncthreads();
  for (int d = 1; d < NT; d <<= 1) {
    const int32_t v = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const int32_t incl = scan[tid], excl = incl - (a + b);
  if (excl <= rank && rank < incl) {
    const bool first = rank < excl + a;
    res[0] = first ? 2 * tid : 2 * tid + 1;
    res[1] = first ? rank - excl : rank - excl - a;
  }
  __syncthreads();
  *idx = res[0];
  *rem = res[1];
  __syncthreads();
}

__device__ inline uint64_t block_max(uint64_t* red, uint64_t v) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int step = NT / 2; step > 0; step >>= 1) {
    if (tid < step && red[tid + step] > red[tid]) red[tid] = red[tid + step];
    __syncthreads();
  }
  const uint64_t best = red[0];
  __syncthreads();
  return best;
}

// whether bin b lies within `reach` bins of one of the earlier picks pk[0 .. npk) of its strand (pk in LDS, npk uniform)
__device__ __forceinline__ bool suppressed(const int32_t* pk, int32_t npk, int32_t reach, int32_t b) {
  for (int32_t i = 0; i < npk; ++i) {
    const int32_t d = b - pk[i];
    if (d <= reach && -d <= reach) return true;
  }
  return false;
}

// the largest (score, -bin) over the hits of one strand; 0 without a hit (a hit scores at least 1).  With SUP the hits of a
// suppressed bin are skipped (seed_candidates_kernel).
template <bool SUP>
__device__ inline uint64_t strand_best(const SeedParams& p, const int2* kc, const int32_t* h, int32_t nk, const int32_t* pk = nullptr,
                                       int32_t npk = 0, int32_t reach = 0) {
  uint64_t best = 0;
  int32_t last = -1;
  for (int32_t r = threadIdx.x; r < nk; r += NT) {
    const int2 e = kc[r];
    for (int32_t t = 0; t < e.y; ++t) {
      const int32_t b = (p.idx_pos[e.x + t] - r + p.off) >> SHIFT;
      if (b == last) continue;
      last = b;
      if (SUP && suppressed(pk, npk, reach, b)) continue;
      const uint64_t key = ((uint64_t)(uint32_t)(counter(h + b) + counter(h + b + 1)) << 32) | (uint32_t)(0x7FFFFFFF - b);
      best = key > best ? key : best;
    }
  }
  return best;
}

// whether read position r of the strand has a hit on the diagonal delta
__device__ inline int32_t on_diagonal(const SeedParams& p, const int2* kc, int32_t r, int32_t nk, int32_t delta) {
  if (r >= nk) return 0;
  const int2 e = kc[r];
  for (int32_t t = 0; t < e.y; ++t)
    if (p.idx_pos[e.x + t] - r == delta) return 1;
  return 0;
}

// pass 1: (first, count) of every k-mer position of both strands into kc0, and 1 added to the bin of each hit in h0
__device__ inline void count_pass(const SeedParams& p, const uint8_t* a, int32_t nk, int2* kc0, int32_t* h0) {
  const int tid = threadIdx.x;
  const int32_t chunk = (nk + NT - 1) / NT;
  const int32_t p0 = imin(tid * chunk, nk), p1 = imin(p0 + chunk, nk);
  uint32_t fwd = 0, rev = 0;
  int32_t run = 0;
  for (int32_t i = p0; p0 < p1 && i < p1 + K - 1; ++i) {
    const uint32_t c = a[i];
    run = c > 3 ? 0 : run + 1;
    fwd = ((fwd << 2) | (c & 3)) & 0x3FFFFFFFu;
    rev = (rev >> 2) | ((3 - (c & 3)) << 28);
    if (i < p0 + K - 1) continue;
    const int32_t r0 = i - (K - 1), r1 = nk - 1 - r0;
    const bool ok = run >= K;
    const int2 e0 = ok ? lookup(p.idx_val, p.n_index, fwd) : make_int2(0, 0);
    const int2 e1 = ok ? lookup(p.idx_val, p.n_index, rev) : make_int2(0, 0);
    kc0[r0] = e0;
    kc0[p.kc_stride + r1] = e1;
    for (int32_t t = 0; t < e0.y; ++t) atomicAdd(h0 + ((p.idx_pos[e0.x + t] - r0 + p.off) >> SHIFT), 1);
    for (int32_t t = 0; t < e1.y; ++t) atomicAdd(h0 + p.nbins + ((p.idx_pos[e1.x + t] - r1 + p.off) >> SHIFT), 1);
  }
}

// pass 3 over one strand: the histogram dh (LDS, 512 counters) of delta over bins beta and beta + 1; with FAR also this thread's
// largest score of a bin more than `reach` bins from beta.  Clears dh first; the caller synchronises after.
template <bool FAR>
__device__ inline int32_t delta_pass(const SeedParams& p, const int2* kcw, const int32_t* hw, int32_t nk, int32_t beta, int32_t reach, int32_t* dh) {
  const int tid = threadIdx.x;
  dh[tid] = 0;
  dh[tid + NT] = 0;
  __syncthreads();
  int32_t far = 0;
  for (int32_t r = tid; r < nk; r += NT) {
    const int2 e = kcw[r];
    for (int32_t t = 0; t < e.y; ++t) {
      const int32_t d = p.idx_pos[e.x + t] - r + p.off, b = d >> SHIFT;
      if (b == beta || b == beta + 1) atomicAdd(dh + (d - (beta << SHIFT)), 1);
      if (FAR && (b - beta > reach || beta - b > reach)) far = imax(far, counter(hw + b) + counter(hw + b + 1));
    }
  }
  return far;
}

// pass 4: the j-th read position with a hit on the diagonal delta, or -1 when the counters do not reach it
__device__ inline int32_t diagonal_hit(const SeedParams& p, const int2* kcw, int32_t nk, int32_t delta, int32_t j, int32_t* dh, int32_t* scan,
                                       int32_t* res) {
  const int tid = threadIdx.x;
  int32_t r_star = -1;
  dh[tid] = 0;
  dh[tid + NT] = 0;
  __syncthreads();
  for (int32_t r = tid; r < nk; r += NT)
    if (on_diagonal(p, kcw, r, nk, delta)) atomicAdd(dh + (r >> SHIFT), 1);
  __syncthreads();
  int32_t block, j2;
  rank_find(dh, scan, res, j, &block, &j2);
  if (block >= 0) {
    dh[tid] = on_diagonal(p, kcw, block * NT + tid, nk, delta);
    dh[tid + NT] = 0;
    __syncthreads();
    int32_t at, rest;
    rank_find(dh, scan, res, j2, &at, &rest);
    if (at >= 0) r_star = block * NT + at;
  }
  return r_star;
}

// pass 5: clear the counters of every bin that holds a hit
__device__ inline void clear_pass(const SeedParams& p, const int2* kc0, int32_t* h0, int32_t nk) {
  for (int s = 0; s < 2; ++s) {
    const int2* kcs = kc0 + s * p.kc_stride;
    int32_t* hs = h0 + s * p.nbins;
    for (int32_t r = threadIdx.x; r < nk; r += NT) {
      const int2 e = kcs[r];
      for (int32_t t = 0; t < e.y; ++t) counter_clear(hs + ((p.idx_pos[e.x + t] - r + p.off) >> SHIFT));
    }
  }
}

__global__ __launch_bounds__(CHIRON_SEED_THREADS) void seed_kernel(SeedParams p) {
  __shared__ int32_t dh[SPAN];
  __shared__ int32_t scan[NT];
  __shared__ int32_t res[2];
  __shared__ uint64_t red[NT];
  const int tid = threadIdx.x;
  int2* const kc0 = p.kc + (int64_t)blockIdx.x * 2 * p.kc_stride;
  int32_t* const h0 = p.hist + (int64_t)blockIdx.x * 2 * p.nbins;
  for (int64_t q = blockIdx.x; q < p.reads; q += gridDim.x) {
    const SeedRead rd = p.read[q];
    const int32_t n = rd.n, nk = n >= K ? n - K + 1 : 0;
    // 1: lookup and count
    count_pass(p, p.codes + rd.start, nk, kc0, h0);
    phase_sync();
    // 2: the winner
    const uint64_t best0 = block_max(red, strand_best<false>(p, kc0, h0, nk));
    const uint64_t best1 = block_max(red, strand_best<false>(p, kc0 + p.kc_stride, h0 + p.nbins, nk));
    const int32_t w = (best1 >> 32) > (best0 >> 32) ? 1 : 0;                  // strand 0 wins a tie
    const uint64_t bestw = w ? best1 : best0;
    const int32_t votes = (int32_t)(bestw >> 32);
    int32_t second = (int32_t)((w ? best0 : best1) >> 32);
    if (votes == 0) {                                                           // no hit on either strand: nothing to clear
      if (tid == 0) {
        int32_t* o = p.out + q * 5;
        o[0] = o[1] = o[2] = o[3] = o[4] = 0;
      }
      continue;
    }
    const int32_t beta = 0x7FFFFFFF - (int32_t)(uint32_t)bestw;
    const int2* const kcw = kc0 + w * p.kc_stride;
    // 3: the far maximum and the deltas of the winning two bins
    const int32_t far = delta_pass<true>(p, kcw, h0 + w * p.nbins, nk, beta, (n >> SHIFT) + 2, dh);
    second = imax(second, (int32_t)block_max(red, (uint64_t)(uint32_t)far));
    int32_t dl, j;
    rank_find(dh, scan, res, (votes - 1) / 2, &dl, &j);
    const int32_t delta = (beta << SHIFT) + dl - p.off;
    // 4: the j-th read position with a hit on that diagonal
    const int32_t r_star = dl >= 0 ? diagonal_hit(p, kcw, nk, delta, j, dh, scan, res) : -1;
    // 5: clear the counters of every bin that holds a hit
    clear_pass(p, kc0, h0, nk);
    if (tid == 0) {
      int32_t* o = p.out + q * 5;
      o[0] = r_star >= 0 ? votes : -1;
      o[1] = second;
      o[2] = w;
      o[3] = delta;
      o[4] = delta + r_star;
    }
    phase_sync();
  }
}

// Up to max_cand candidates a read, equal to map.vote_top: passes 1 and 5 once, passes 2 to 4 once a pick.  A pick at bin beta
// suppresses the bins of its strand within n / 256 + 2 of beta for the later winner passes; the picks are the same for every
// thread, so they live in LDS (pk) and in uniform counts.  out: [reads][1 + 4 max_cand]: the count, then (votes, strand, delta, g)
// of each pick, zeros from the count on; votes -1 where a rank fell off the counters.
__global__ __launch_bounds__(CHIRON_SEED_THREADS) void seed_candidates_kernel(SeedParams p, int32_t max_cand, int32_t min_score) {
  __shared__ int32_t dh[SPAN];
  __shared__ int32_t scan[NT];
  __shared__ int32_t res[2];
  __shared__ uint64_t red[NT];
  __shared__ int32_t pk[2][CHIRON_SEED_MAX_CANDIDATES];
  const int tid = threadIdx.x;
  int2* const kc0 = p.kc + (int64_t)blockIdx.x * 2 * p.kc_stride;
  int32_t* const h0 = p.hist + (int64_t)blockIdx.x * 2 * p.nbins;
  for (int64_t q = blockIdx.x; q < p.reads; q += gridDim.x) {
    const SeedRead rd = p.read[q];
    const int32_t n = rd.n, nk = n >= K ? n - K + 1 : 0, reach = (n >> SHIFT) + 2;
    int32_t* const o = p.out + q * (1 + 4 * max_cand);
    count_pass(p, p.codes + rd.start, nk, kc0, h0);
    phase_sync();
    int32_t np0 = 0, np1 = 0, count = 0;
    bool any = false;
    while (count < max_cand) {
      const uint64_t best0 = block_max(red, strand_best<true>(p, kc0, h0, nk, pk[0], np0, reach));
      const uint64_t best1 = block_max(red, strand_best<true>(p, kc0 + p.kc_stride, h0 + p.nbins, nk, pk[1], np1, reach));
      const int32_t w = (best1 >> 32) > (best0 >> 32) ? 1 : 0;
      const uint64_t bestw = w ? best1 : best0;
      const int32_t votes = (int32_t)(bestw >> 32);
      if (count == 0) any = votes > 0;
      if (votes < min_score) break;                                            // min_score >= 1: the end of the hits as well
      const int32_t beta = 0x7FFFFFFF - (int32_t)(uint32_t)bestw;
      const int2* const kcw = kc0 + w * p.kc_stride;
      delta_pass<false>(p, kcw, h0 + w * p.nbins, nk, beta, reach, dh);
      __syncthreads();
      int32_t dl, j;
      rank_find(dh, scan, res, (votes - 1) / 2, &dl, &j);
      const int32_t delta = (beta << SHIFT) + dl - p.off;
      const int32_t r_star = dl >= 0 ? diagonal_hit(p, kcw, nk, delta, j, dh, scan, res) : -1;
      if (tid == 0) {
        int32_t* oc = o + 1 + 4 * count;
        oc[0] = r_star >= 0 ? votes : -1;
        oc[1] = w;
        oc[2] = delta;
        oc[3] = delta + r_star;
        pk[w][w ? np1 : np0] = beta;
      }
      np0 += 1 - w;
      np1 += w;
      ++count;
      __syncthreads();
    }
    if (any) clear_pass(p, kc0, h0, nk);                                       // without a hit there is nothing to clear
    if (tid == 0) {
      o[0] = count;
      for (int32_t i = 1 + 4 * count; i < 1 + 4 * max_cand; ++i) o[i] = 0;
    }
    if (any) phase_sync();
  }
}

struct SeedLayout {
  size_t val, pos, codes, read, out, kc, hist, bytes;
  int64_t kc_stride, nbins;
  int32_t off;
  int groups;
};

// out_words: int32 results a read (5 for seed_kernel, 1 + 4 max_cand for seed_candidates_kernel)
chiron_status seed_layout(const char* who, int64_t n_index, int64_t genome_len, int64_t reads, int64_t max_read, int64_t total_bases,
                          int64_t out_words, SeedLayout* l) {
  if (n_index < 0 || genome_len < 0 || reads < 0 || max_read < 0 || total_bases < 0)
    return set_error(CHIRON_ERR_INVALID, "%s: negative n_index / genome_len / reads / max_read / total_bases", who);
  if (reads > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld reads in one call, at most 2^24", who, (long long)reads);
  if (max_read > CHIRON_INFIX_MAX_READ)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: a read of %lld bases, the kernel takes at most %d", who, (long long)max_read, CHIRON_INFIX_MAX_READ);
  if (genome_len > CHIRON_SEED_MAX_GENOME)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: a genome of %lld bases, at most %lld keep every diagonal in 32 bits", who, (long long)genome_len,
                     (long long)CHIRON_SEED_MAX_GENOME);
  if (n_index > 0x7FFFFFFF) return set_error(CHIRON_ERR_OVERFLOW, "%s: an index of %lld entries, at most 2^31 - 1", who, (long long)n_index);
  if (total_bases > reads * (int64_t)CHIRON_INFIX_MAX_READ)
    return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld bases in %lld reads of at most %d", who, (long long)total_bases, (long long)reads,
                     CHIRON_INFIX_MAX_READ);
  l->groups = (int)(reads < CHIRON_SEED_MAX_GROUPS ? reads : CHIRON_SEED_MAX_GROUPS);
  l->kc_stride = max_read;
  l->off = (int32_t)((max_read + CHIRON_SEED_BIN - 1) / CHIRON_SEED_BIN * CHIRON_SEED_BIN);
  l->nbins = (genome_len + l->off) / CHIRON_SEED_BIN + 2;       // the highest bin that can hold a hit, and the one above it
  size_t at = 0;
  l->val = at, at += up256((size_t)n_index * 4);
  l->pos = at, at += up256((size_t)n_index * 4);
  l->codes = at, at += up256((size_t)total_bases + 1);
  l->read = at, at += up256((size_t)reads * sizeof(SeedRead));
  l->out = at, at += up256((size_t)reads * (size_t)out_words * 4);
  l->kc = at, at += up256((size_t)l->groups * 2 * (size_t)l->kc_stride * sizeof(int2));
  l->hist = at, at += up256((size_t)l->groups * 2 * (size_t)l->nbins * 4);
  l->bytes = at;
  return CHIRON_OK;
}

chiron_status check_candidates(const char* who, int32_t max_cand, int32_t min_score) {
  if (max_cand < 1 || max_cand > CHIRON_SEED_MAX_CANDIDATES)
    return set_error(CHIRON_ERR_INVALID, "%s: max_cand %d outside 1 .. %d", who, max_cand, CHIRON_SEED_MAX_CANDIDATES);
  if (min_score < 1) return set_error(CHIRON_ERR_INVALID, "%s: min_score %d below 1", who, min_score);
  return CHIRON_OK;
}

// What chiron_seed_reads and chiron_seed_candidates share.  check(): every refusal that needs no device, in one order, and the
// reads packed for the kernel; *done when the answer needs no device (no reads, or an empty index).  run(): the copies in, the
// launch and the results back into out ([reads][out_words]), stream synchronised.
struct SeedCall {
  const char* who;
  const uint32_t* idx_val;
  const int32_t* idx_pos;
  int64_t n_index, genome_len;
  const uint8_t* codes;
  const int64_t* read_off;
  int64_t reads;
  uint32_t flags;
  int64_t out_words;
  SeedLayout l;
  std::vector<uint8_t> packed;
  std::vector<SeedRead> recs;
  std::vector<int32_t> out;

  chiron_status check(bool outputs_given, bool* done) {
    *done = false;
    if (reads < 0) return set_error(CHIRON_ERR_INVALID, "%s: reads %lld", who, (long long)reads);
    if (n_index < 0 || genome_len < 0)
      return set_error(CHIRON_ERR_INVALID, "%s: negative n_index %lld or genome_len %lld", who, (long long)n_index, (long long)genome_len);
    if (flags) return set_error(CHIRON_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
    if (reads == 0) {
      *done = true;
      return CHIRON_OK;
    }
    if (reads > MAX_BATCH_ITEMS) return set_error(CHIRON_ERR_OVERFLOW, "%s: %lld reads in one call, at most 2^24", who, (long long)reads);
    if (!read_off || !outputs_given || (n_index > 0 && (!idx_val || !idx_pos))) return set_error(CHIRON_ERR_INVALID, "%s: null operand", who);
    int64_t max_read = 0, total = 0;
    chiron_status st = check_offsets(who, "read", "read", "bases", read_off, reads, CHIRON_INFIX_MAX_READ, &max_read, &total);
    if (st) return st;
    if (total > 0 && !codes) return set_error(CHIRON_ERR_INVALID, "%s: null codes", who);
    if ((st = seed_layout(who, n_index, genome_len, reads, max_read, total, out_words, &l))) return st;
    // the index: sorted, and every position that of a whole k-mer inside the genome (what bounds the kernel's bin indices)
    for (int64_t i = 0; i < n_index; ++i) {
      if (i > 0 && idx_val[i] < idx_val[i - 1])
        return set_error(CHIRON_ERR_INVALID, "%s: the index is not sorted: idx_val[%lld] = %u below its predecessor %u", who, (long long)i, idx_val[i],
                         idx_val[i - 1]);
      if (idx_pos[i] < 0 || (int64_t)idx_pos[i] > genome_len - CHIRON_SEED_K)
        return set_error(CHIRON_ERR_INVALID, "%s: idx_pos[%lld] = %d outside the k-mer positions 0 .. %lld of the genome", who, (long long)i, idx_pos[i],
                         (long long)(genome_len - CHIRON_SEED_K));
    }
    packed.assign((size_t)total + 1, 0);
    recs.resize((size_t)reads);
    int64_t at = 0;
    for (int64_t q = 0; q < reads; ++q) {
      const int64_t len = read_off[q + 1] - read_off[q];
      recs[q] = {at, (int32_t)len, 0};
      for (int64_t i = 0; i < len; ++i) {
        const uint8_t c = codes[read_off[q] + i];
        if (c > 4) return set_error(CHIRON_ERR_INVALID, "%s: code %d at %lld of read %lld outside 0..4", who, (int)c, (long long)i, (long long)q);
        packed[at + i] = c;
      }
      at += len;
    }
    *done = n_index == 0;                                // an empty index: nothing can hit, and no device is needed to say so
    return CHIRON_OK;
  }

  // launch(params, groups, stream) starts the kernel
  template <typename Launch>
  chiron_status run(int32_t device_id, void* workspace, void* stream_, Launch launch) {
    chiron_status st;
    if ((st = use_device_workspace(who, device_id, workspace))) return st;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    if (hipMemcpyAsync(ws + l.val, idx_val, (size_t)n_index * 4, hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(ws + l.pos, idx_pos, (size_t)n_index * 4, hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(ws + l.codes, packed.data(), packed.size(), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(ws + l.read, recs.data(), recs.size() * sizeof(SeedRead), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemsetAsync(ws + l.hist, 0, (size_t)l.groups * 2 * (size_t)l.nbins * 4, stream) != hipSuccess)
      return set_error(CHIRON_ERR_DEVICE, "%s: copying the index and the reads to the device failed", who);
    SeedParams p;
    p.idx_val = (const uint32_t*)(ws + l.val);
    p.idx_pos = (const int32_t*)(ws + l.pos);
    p.n_index = (int32_t)n_index;
    p.codes = (const uint8_t*)(ws + l.codes);
    p.read = (const SeedRead*)(ws + l.read);
    p.reads = reads;
    p.kc = (int2*)(ws + l.kc);
    p.kc_stride = l.kc_stride;
    p.hist = (int32_t*)(ws + l.hist);
    p.nbins = l.nbins;
    p.off = l.off;
    p.out = (int32_t*)(ws + l.out);
    launch(p, l.groups, stream);
    if (hipGetLastError() != hipSuccess) return set_error(CHIRON_ERR_DEVICE, "%s: launch failed", who);
    out.resize((size_t)reads * (size_t)out_words);
    if (hipMemcpyAsync(out.data(), ws + l.out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
      return set_error(CHIRON_ERR_DEVICE, "%s: the seeding kernel failed (%s)", who, hipGetErrorString(hipGetLastError()));
    return CHIRON_OK;
  }
};

}  // namespace

}  // namespace chiron

using namespace chiron;

extern "C" chiron_status chiron_seed_workspace_size(int64_t n_index, int64_t genome_len, int64_t reads, int64_t max_read, int64_t total_bases,
                                                    size_t* bytes) {
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "chiron_seed_workspace_size: null bytes");
  SeedLayout l;
  chiron_status st = seed_layout("chiron_seed_workspace_size", n_index, genome_len, reads, max_read, total_bases, 5, &l);
  if (st) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_seed_candidates_workspace_size(int64_t n_index, int64_t genome_len, int64_t reads, int64_t max_read,
                                                               int64_t total_bases, int32_t max_cand, size_t* bytes) {
  const char* const who = "chiron_seed_candidates_workspace_size";
  if (!bytes) return set_error(CHIRON_ERR_INVALID, "%s: null bytes", who);
  chiron_status st = check_candidates(who, max_cand, 1);
  if (st) return st;
  SeedLayout l;
  if ((st = seed_layout(who, n_index, genome_len, reads, max_read, total_bases, 1 + 4 * (int64_t)max_cand, &l))) return st;
  *bytes = l.bytes;
  return CHIRON_OK;
}

extern "C" chiron_status chiron_seed_reads(int32_t device_id, const uint32_t* idx_val, const int32_t* idx_pos, int64_t n_index, int64_t genome_len,
                                           const uint8_t* codes, const int64_t* read_off, int64_t reads, uint32_t flags, int32_t* votes_out,
                                           int32_t* second_out, int32_t* strand_out, int64_t* delta_out, int64_t* g_out, void* workspace,
                                           void* stream_) {
  SeedCall c{"chiron_seed_reads", idx_val, idx_pos, n_index, genome_len, codes, read_off, reads, flags, 5};
  bool done;
  chiron_status st = c.check(votes_out && second_out && strand_out && delta_out && g_out, &done);
  if (st) return st;
  if (done) {
    for (int64_t q = 0; q < reads; ++q) votes_out[q] = second_out[q] = strand_out[q] = delta_out[q] = g_out[q] = 0;
    return CHIRON_OK;
  }
  st = c.run(device_id, workspace, stream_, [](const SeedParams& p, int groups, hipStream_t stream) {
    hipLaunchKernelGGL(seed_kernel, dim3(groups), dim3(CHIRON_SEED_THREADS), 0, stream, p);
  });
  if (st) return st;
  const std::vector<int32_t>& out = c.out;
  for (int64_t q = 0; q < reads; ++q) {
    if (out[q * 5] < 0) return set_error(CHIRON_ERR_STATE, "%s: the counters of read %lld do not add up to its votes", c.who, (long long)q);
    votes_out[q] = out[q * 5];
    second_out[q] = out[q * 5 + 1];
    strand_out[q] = out[q * 5 + 2];
    delta_out[q] = out[q * 5 + 3];
    g_out[q] = out[q * 5 + 4];
  }
  return CHIRON_OK;
}

extern "C" chiron_status chiron_seed_candidates(int32_t device_id, const uint32_t* idx_val, const int32_t* idx_pos, int64_t n_index,
                                                int64_t genome_len, const uint8_t* codes, const int64_t* read_off, int64_t reads,
                                                int32_t max_cand, int32_t min_score, uint32_t flags, int32_t* count_out, int32_t* votes_out,
                                                int32_t* strand_out, int64_t* delta_out, int64_t* g_out, void* workspace, void* stream_) {
  const char* const who = "chiron_seed_candidates";
  chiron_status st = check_candidates(who, max_cand, min_score);
  if (st) return st;
  const int64_t words = 1 + 4 * (int64_t)max_cand;
  SeedCall c{who, idx_val, idx_pos, n_index, genome_len, codes, read_off, reads, flags, words};
  bool done;
  if ((st = c.check(count_out && votes_out && strand_out && delta_out && g_out, &done))) return st;
  if (done) {
    for (int64_t q = 0; q < reads; ++q) count_out[q] = 0;
    for (int64_t i = 0; i < reads * max_cand; ++i) votes_out[i] = strand_out[i] = delta_out[i] = g_out[i] = 0;
    return CHIRON_OK;
  }
  st = c.run(device_id, workspace, stream_, [=](const SeedParams& p, int groups, hipStream_t stream) {
    hipLaunchKernelGGL(seed_candidates_kernel, dim3(groups), dim3(CHIRON_SEED_THREADS), 0, stream, p, max_cand, min_score);
  });
  if (st) return st;
  const std::vector<int32_t>& out = c.out;
  for (int64_t q = 0; q < reads; ++q) {
    const int32_t* o = out.data() + q * words;
    count_out[q] = o[0];
    for (int32_t k = 0; k < max_cand; ++k) {
      if (o[1 + 4 * k] < 0)
        return set_error(CHIRON_ERR_STATE, "%s: the counters of read %lld do not add up to the votes of its pick %d", who, (long long)q, k);
      const int64_t at = q * max_cand + k;
      votes_out[at] = o[1 + 4 * k];
      strand_out[at] = o[2 + 4 * k];
      delta_out[at] = o[3 + 4 * k];
      g_out[at] = o[4 + 4 * k];
    }
  }
  return CHIRON_OK;
}
