// sw_seed_kernel.h — the seed stage in front of the chained prefix filter (host_pipeline.h prefix_seeded).
//
// A SEED is k consecutive code bytes of a read, taken at the disjoint offsets 0, k, 2k, ... (seeds of period <= k / 2 left out).  The batch's seeds sit in an open-addressing
// table {hash, seed id} (linear probing; equal seeds of different reads are entries of their own behind each other), and one pass over
// the range of the reference rolls the same hash over every window of k codes: a table match is compared letter by letter, and a true
// match appends {start = position - offset, offset} to the read's hit list.  A list holds kSeedHitCap hits; the count goes on beyond
// it, exactly (the host drops a read whose list overflowed: which hits it kept depends on the order of the atomics, the count does not).
//
// The table is the L2's (8 bytes per slot at a load of at most 1/8: 2 MB for the 20 480 seeds of 2048 reads of 150 bp); a bit per table bucket sits in LDS, and a window whose home bucket is empty — most of them —
// never leaves the CU.  Plain C++: vector loads, vector atomics, plain stores.
//
// Bounds: thread T owns the positions [T * kSeedStretch, (T + 1) * kSeedStretch) of the range and probes only those <= n - k, so the
// last code it reads is that of column n - 1; a range shorter than k probes nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace mi355sw {

constexpr int kSeedStretch = 64;                 // positions of the range per thread
constexpr int kSeedThreads = 256;                // threads per workgroup: a workgroup spans kSeedThreads * kSeedStretch = 16384 positions
constexpr int kSeedHitCap = 32;                  // hits listed per read
constexpr int kSeedMinPerRead = 4;               // seeds the shortest read must hold
constexpr int kSeedMaxK = 32;
constexpr int kSeedBitsLog2Max = 18;             // bucket bits in LDS: at most 2^18 bits = 32 KB
constexpr uint32_t kSeedBase = 0x01000193u;      // the polynomial's base (odd)
constexpr uint32_t kSeedMix = 0x9E3779B1u;       // slot = (hash * kSeedMix) >> (32 - bits)
constexpr uint32_t kSeedEmpty = 0xFFFFFFFFu;     // seed id of an empty slot

// hash of c[0 .. k): sum (c[i] + 1) B^(k - 1 - i) mod 2^32, so that it rolls: h' = h B + (c[k] + 1) - (c[0] + 1) B^k
__host__ __device__ inline uint32_t seed_hash_push(uint32_t h, uint32_t c) { return h * kSeedBase + c + 1u; }
__host__ __device__ inline uint32_t seed_hash_roll(uint32_t h, uint32_t c_out, uint32_t c_in, uint32_t bk) {
  return h * kSeedBase + c_in + 1u - (c_out + 1u) * bk;
}
__host__ __device__ inline uint32_t seed_slot(uint32_t h, int bits) { return (h * kSeedMix) >> (32 - bits); }
inline uint32_t seed_hash(const uint8_t *c, int k) {
  uint32_t h = 0;
  for (int i = 0; i < k; ++i) h = seed_hash_push(h, c[i]);
  return h;
}
inline uint32_t seed_base_pow(int k) {
  uint32_t b = 1;
  for (int i = 0; i < k; ++i) b *= kSeedBase;
  return b;
}

// The seed length for reads of at least `minlen` letters over `letters` distinct letters against n columns: the smallest k with
// letters^k >= (minlen / k) n — fewer than one chance hit per read expected under uniform letters — that leaves kSeedMinPerRead
// seeds in the shortest read; 0: there is none (the stage is not used).  DNA, 150 bp, 50 Mbp: 4^15 = 1.07e9 >= 10 * 5e7, k = 15.
inline int seed_k(int letters, int minlen, int64_t n) {
  if (letters < 2 || n < 1) return 0;
  for (int k = 1; k <= kSeedMaxK; ++k) {
    const int64_t per_read = minlen / k;
    if (per_read < kSeedMinPerRead) return 0;
    const double want = (double)per_read * (double)n;
    double have = 1.0;
    for (int i = 0; i < k && have < want; ++i) have *= (double)letters;
    if (have >= want) return k;
  }
  return 0;
}

// A seed that repeats itself with a period of at most k / 2 letters (poly-A, a microsatellite) is left out, as every seed-and-extend
// mapper masks such seeds: it says nothing about where the read belongs and hits every run of its kind at every position (bench.py's
// repeat-rich reference: 25 million hits for some twenty such reads, a scan of 28 ms instead of 0.4).
inline bool seed_periodic(const uint8_t *c, int k) {
  for (int p = 1; p <= k / 2; ++p) {
    bool same = true;
    for (int i = 0; i + p < k && same; ++i) same = c[i] == c[i + p];
    if (same) return true;
  }
  return false;
}

// The batch's seeds and their table, built on the host.
struct SeedTable {
  int k = 0, bits = 0, bucket_log2 = 0;          // seed length, log2 of the slots, log2 of the LDS bits (<= bits)
  uint32_t bk = 0;                               // kSeedBase^k
  std::vector<uint8_t> codes;                    // [nseeds][k]
  std::vector<int32_t> read, off;                // [nseeds]
  std::vector<uint32_t> slots;                   // [2 << bits]: {hash, seed id}
  std::vector<uint32_t> bucket;                  // [1 << (bucket_log2 - 5)] bit b: some slot with (slot >> (bits - bucket_log2)) == b is taken
  size_t nseeds() const { return read.size(); }
};
// x(id) = bytes + off[id], len[id] letters; code_of[letter] < 0: the reference does not hold that letter, a seed with it is left out
// false: more seeds than half of the largest table (2^26 slots) — nothing is inserted
inline bool seed_table_build(SeedTable &t, int k, const uint8_t *bytes, const int64_t *off, const int32_t *len, const int32_t *ids, size_t nids,
                             const int *code_of) {
  t = SeedTable();
  t.k = k; t.bk = seed_base_pow(k);
  for (size_t r = 0; r < nids; ++r) {
    const int id = ids[r];
    const uint8_t *x = bytes + off[id];
    for (int o = 0; o + k <= len[id]; o += k) {
      bool known = true;
      for (int i = 0; i < k; ++i) known = known && code_of[x[o + i]] >= 0;
      if (!known || seed_periodic(x + o, k)) continue;
      for (int i = 0; i < k; ++i) t.codes.push_back((uint8_t)code_of[x[o + i]]);
      t.read.push_back(id); t.off.push_back(o);
    }
  }
  const size_t n = t.nseeds();
  t.bits = 10;
  while (((size_t)1 << t.bits) < 8 * n && t.bits < 26) ++t.bits;        // load <= 1/8 (at 2^26 slots: up to 1/2)
  if (2 * n > ((size_t)1 << t.bits)) return false;                      // (the probe loop below needs free slots to end)
  t.bucket_log2 = std::min(t.bits, kSeedBitsLog2Max);
  t.slots.assign((size_t)2 << t.bits, kSeedEmpty);
  t.bucket.assign((size_t)1 << (t.bucket_log2 - 5), 0u);
  const uint32_t mask = ((uint32_t)1 << t.bits) - 1u;
  for (size_t s = 0; s < n; ++s) {
    const uint32_t h = seed_hash(t.codes.data() + s * (size_t)k, k);
    uint32_t at = seed_slot(h, t.bits);
    while (t.slots[2 * (size_t)at + 1] != kSeedEmpty) at = (at + 1) & mask;
    t.slots[2 * (size_t)at] = h; t.slots[2 * (size_t)at + 1] = (uint32_t)s;
    const uint32_t b = at >> (t.bits - t.bucket_log2);
    t.bucket[b >> 5] |= 1u << (b & 31);
  }
  return true;
}

struct SeedHit { int64_t start; int32_t off; };
inline bool operator<(const SeedHit &a, const SeedHit &b) { return a.start != b.start ? a.start < b.start : a.off < b.off; }
// The cluster of one read's hits (any order): for every hit as the anchor, the hits whose start lies in [anchor, anchor + width]; the
// anchor with the most distinct seed offsets wins, ties go to the lowest start.  false: no hit.  lo / hi: the cluster's starts.
inline bool seed_cluster(std::vector<SeedHit> hits, int64_t width, int64_t &lo, int64_t &hi, int &distinct) {
  if (hits.empty()) return false;
  std::sort(hits.begin(), hits.end());
  distinct = 0;
  for (size_t a = 0; a < hits.size(); ++a) {
    if (a > 0 && hits[a].start == hits[a - 1].start) continue;        // (the same anchor)
    std::vector<int32_t> offs;
    size_t b = a;
    for (; b < hits.size() && hits[b].start <= hits[a].start + width; ++b) offs.push_back(hits[b].off);
    std::sort(offs.begin(), offs.end());
    const int d = (int)(std::unique(offs.begin(), offs.end()) - offs.begin());
    if (d > distinct) { distinct = d; lo = hits[a].start; hi = hits[b - 1].start; }
  }
  return true;
}

// u of lemma L21: the seeds of every read that entered the table, by read id.  Seeds with a letter the reference
// does not hold and periodic seeds are not in it, which only lowers u.
inline void seed_usable(const SeedTable &t, size_t nq, std::vector<uint32_t> &u) {
  u.assign(nq, 0u);
  for (int32_t r : t.read) if (r >= 0 && (size_t)r < nq) ++u[(size_t)r];
}
// The rule of L21 for a read of deficit d = smax m - B0 with u seeds in the table: every alignment of score >= B0 breaks at most
// floor(d / c) seeds, c = min(g, smax), so it keeps an intact one while that is below u.  (Each way to break a seed must cost c or
// more; a table whose mismatches can score above smax - c is the caller's to leave out.)
inline bool seed_certify_ok(int64_t d, int64_t smax, int64_t g, int64_t u) {
  if (d < 0 || smax <= 0 || g <= 0 || u <= 0) return false;
  return d / std::min(g, smax) < u;
}
// ... and the end columns (0-based, inside [0, n)) of such an alignment through the intact seed of the hit `start` (position - offset):
// start + m - 1, moved left by at most floor(d / c) clipped or inserted read letters and right by at most floor(d / g) reference
// letters against a gap.  false: the interval has no column of the range.
inline bool seed_certify_window(int64_t start, int64_t m, int64_t d, int64_t smax, int64_t g, int64_t n, int64_t &lo, int64_t &hi) {
  if (d < 0 || smax <= 0 || g <= 0 || m <= 0 || n <= 0) return false;
  const int64_t end = start + m - 1;
  lo = std::max<int64_t>(0, end - d / std::min(g, smax));
  hi = std::min<int64_t>(n - 1, end + d / g);
  return lo <= hi;
}

struct SeedArgs {
  const uint8_t *codes;      // reference codes of the RANGE's first column
  int64_t n;                 // columns of the range
  int k;
  uint32_t bk;               // kSeedBase^k
  const uint2 *slots;        // [1 << bits] {hash, seed id}
  int bits, bucket_log2;
  const uint32_t *bucket;    // [1 << (bucket_log2 - 5)]
  const uint8_t *seed_codes; // [nseeds][k]
  const int32_t *seed_read;  // [nseeds]
  const int32_t *seed_off;   // [nseeds]
  unsigned int *count;       // [nq] hits per read, exact
  int64_t *hit_start;        // [nq][kSeedHitCap] position - offset, relative to the range (may be negative)
  int32_t *hit_off;          // [nq][kSeedHitCap]
};

__global__ __launch_bounds__(kSeedThreads) void sw_seed_scan_kernel(const SeedArgs a) {
  extern __shared__ uint32_t seed_bucket[];
  const int words = 1 << (a.bucket_log2 - 5);
  for (int w = threadIdx.x; w < words; w += kSeedThreads) seed_bucket[w] = a.bucket[w];
  __syncthreads();
  const int64_t last = a.n - a.k;                                    // the last position probed
  const int64_t p0 = ((int64_t)blockIdx.x * kSeedThreads + threadIdx.x) * kSeedStretch;
  if (p0 > last) return;
  const int64_t p1 = p0 + kSeedStretch - 1 < last ? p0 + kSeedStretch - 1 : last;
  const uint32_t mask = ((uint32_t)1 << a.bits) - 1u;
  const int shift = a.bits - a.bucket_log2;
  uint32_t h = 0;
  for (int i = 0; i < a.k; ++i) h = seed_hash_push(h, a.codes[p0 + i]);
  // A read whose list is already full only counts on, and a run of letters can hold its seed at every position (a poly-A read against
  // 500 poly-A runs: 1.4 million hits on ONE counter, tens of ms of serialised atomics).  Such hits are held back and added once per
  // thread and read: the count stays exact, the list is the first kSeedHitCap by the order of the atomics as before.
  int held_q = -1;
  unsigned int held_n = 0;
  for (int64_t p = p0;; ++p) {
    uint32_t at = seed_slot(h, a.bits);
    const uint32_t b = at >> shift;
    if (seed_bucket[b >> 5] >> (b & 31) & 1u) {
      for (uint32_t tries = 0; tries <= mask; ++tries, at = (at + 1) & mask) {
        const uint2 e = a.slots[at];
        if (e.y == kSeedEmpty) break;
        if (e.x != h) continue;
        const uint8_t *s = a.seed_codes + (size_t)e.y * (size_t)a.k;
        bool same = true;
        for (int i = 0; i < a.k && same; ++i) same = s[i] == a.codes[p + i];
        if (!same) continue;
        const int q = a.seed_read[e.y], o = a.seed_off[e.y];
        if (q == held_q) { ++held_n; continue; }
        if (__hip_atomic_load(a.count + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned int)kSeedHitCap) {
          if (held_n) atomicAdd(a.count + held_q, held_n);
          held_q = q; held_n = 1;
          continue;
        }
        const unsigned int c = atomicAdd(a.count + q, 1u);
        if (c < (unsigned int)kSeedHitCap) {
          a.hit_start[(size_t)q * kSeedHitCap + c] = p - (int64_t)o;
          a.hit_off[(size_t)q * kSeedHitCap + c] = o;
        }
      }
    }
    if (p == p1) break;
    h = seed_hash_roll(h, a.codes[p], a.codes[p + a.k], a.bk);       // (p < p1 <= n - k: column p + k exists)
  }
  if (held_n) atomicAdd(a.count + held_q, held_n);
}

}  // namespace mi355sw
