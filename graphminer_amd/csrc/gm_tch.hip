// gm_tch.hip -- triangle counting, the shorter list streamed (gm_tch.hip) against the chunk's DAG rows kept in LDS as ONE HASHED SET of
// (row, id) pairs instead of a sorted copy behind a bit filter.
//
// Why (profiles/r03/tc_rmat22_pmc_summary.txt, section 4.11 of DESIGN.md): tct_kernel issues 66 VALU instructions per 64 streamed
// keys and keeps the SIMDs 0.65 - 1.1 busy.  22 % of the streamed keys of R-MAT-22 ARE common neighbours (30 % on the com-Orkut
// stand-in), 27 % pass the bit filter -- and every one of them is written to the per-wave queue, read back and bisected against
// the sorted LDS copy (8 - 11 dependent LDS reads).  A triangle count needs no position, only membership
// (src/triangle/gpu_kernels/bs_warp_edge.cuh:9-15 counts the matches of a binary search), so the rows are stored as a set:
//   * a bucket is four 32-bit slots (one 16-byte LDS line) holding full ids; there are as many buckets as stage entries;
//   * bucket of (row r, id x) = top bits of x * C  XOR  salt(r), salt(r) = r * 37 mod #buckets: INJECTIVE in the local row (<= 256
//     rows, >= 1024 buckets), so the same id staged for two rows of the chunk sits in two different buckets and a hit is exact --
//     the slot needs no row tag;
//   * lookup = one multiply, one ds_read_b128, four compares whose results stay lane masks in SGPRs, one s_bcnt1: no queue, no
//     compaction, no bisection;
//   * a bucket that got more than four entries (0.4 % of them at this load) carries a marker in its last slot; its surplus
//     entries sit in a list of <= 128 (id, salt) pairs that only the lanes missing in such a bucket consult.  A chunk that overflows
//     the list (adversarial ids) is looked up by bisection of the row in global memory -- slow, exact (tune[6] & GM_T6_HSET_FALLBACK forces it).
// Chunk table, task lists, parts, dequeue order: those of tct_kernel (the kernel is chosen per launch, gm_launch.hip).
#include <type_traits>
#include "gm_flat.h"
#include "gm_tch_rule.h"

namespace gm {

#ifndef GM_TCH_TILES
#define GM_TCH_TILES 4
#endif
constexpr int kTchTiles = GM_TCH_TILES;  // 64-key tiles in flight per wave (long lists, 2048-bucket kernel)
#ifndef GM_TCH_TILES_SMALL
#define GM_TCH_TILES_SMALL 2
#endif
constexpr int kTchTilesSmall = GM_TCH_TILES_SMALL;  // ... 1024-bucket kernel
// ... in the flattened pass of the short lists, per stage (one group ahead is in flight on top).  Chosen in round 4, on the kernel
// before the hub corner and before the peeled steady state -- R-MAT-22 / power law / flat degrees / R-MAT-24 formula 3-motif, ms then:
// 4 tiles 3.02 / 1.08 / 0.86 / 42.9, 8 tiles 3.04 / 1.12 / 0.90 / 42.1 -- and not swept again since: the 1024-bucket kernel holds 79
// of its 80 registers with 4 tiles, the 2048-bucket kernel has the registers for 8
constexpr int kTchFlatTilesSmall = 4, kTchFlatTilesBig = 8;

// lookup lists of at least this many keys are streamed one task at a time, shorter ones flattened 64 to a batch.  Its own threshold
// (kLongList, 192, also sizes the edge supports' masks and the motif trims of the other kernels): with the hub corner on the matrix
// cores the lists of 192 .. 383 keys are streamed faster flattened -- one at a time, a list of two or three tile groups waits for
// its keys with nothing else in flight (R-MAT-22 TC, ms per step: 192: 1.85, 256: 1.73, 384: 1.70, 512: 1.70, 1024: 1.70; R-MAT-24
// formula 3-motif 24.3 -> 21.7 at 384)
#ifndef GM_TCH_LONG_LIST
#define GM_TCH_LONG_LIST 384
#endif
constexpr int kTchLongList = GM_TCH_LONG_LIST;

// (kTchFlatBias, kTchNarrowEntries and the rule that chooses between the narrow and the WIDE key addressing of the flattened pass: gm_tch_rule.h)

constexpr int kTchOvfCap = 128;
constexpr unsigned kTchEmpty = 0xffffffffu, kTchMarker = 0xfffffffeu;  // (ids are < 2^31 - 1)
constexpr unsigned kTchMul = 0x9E3779B1u;

// flattened positions per mark window (a batch of 64 lists below kTchLongList keys: <= 24512, most have far fewer; a longer batch is
// streamed window after window): 8192 beside the 1024-bucket table, 4096 beside the 2048-bucket one (the LDS budget of six / four
// workgroups per CU)
template <int BITWIN>
struct alignas(16) TchWave {
  int2 desc[GM_WAVE];              // per non-empty list of the batch: {key_base - offset among the flattened positions (times four, modulo
                                   // 2^32, in the narrow form: kTchFlatBias), salt of the host row}
  unsigned bits[BITWIN / 32 + 8];  // list-start marks of the flattened positions, one bit each (+ the over-read of the last group)
};

// waves of a workgroup: four on the 1024-bucket table; GM_TCH_WAVES_BIG on the 2048-bucket one (the hosts with rows of 1025 .. 2048 entries)
#ifndef GM_TCH_WAVES_BIG
#define GM_TCH_WAVES_BIG 4
#endif
#ifndef GM_TCH_MIN_WG_BIG
#define GM_TCH_MIN_WG_BIG 4
#endif
template <int STAGE>
constexpr int tch_waves() { return STAGE <= 1024 ? kWavesPerBlock : GM_TCH_WAVES_BIG; }
template <int STAGE>
struct alignas(16) TchLds {
  uint4 table[STAGE];              // buckets of four ids
  int rpl[kMaxChunkVerts + 1];     // row offsets of the chunk's DAG rows (global entry indices)
  int trpl[kMaxChunkVerts + 1];    // row offsets of its task lists
  static constexpr int kBitWindow = STAGE <= 1024 ? 8192 : 4096;
  TchWave<kBitWindow> w[tch_waves<STAGE>()];  // (while the table is built: packed 16-bit fill counters of the buckets)
  int ovf_key[kTchOvfCap];
  int ovf_salt[kTchOvfCap];
  int n_ovf;
  int next_batch;
  unsigned queue_pos;
  int next_group;  // key stream of the short lists: the next group of tiles
};
static_assert(kTchOvfCap == 2 * GM_WAVE, "the surplus list is scanned two entries per lane");

template <int STAGE>
struct TchHash {
  static constexpr int LB = STAGE == 1024 ? 10 : 11;
  static_assert((1 << LB) == STAGE, "one bucket per stage entry");
  static constexpr unsigned kMask = (unsigned)(STAGE - 1) << 4;
  // byte offset of the bucket of (id x, row salt s)
  static __device__ __forceinline__ unsigned bucket(int x, unsigned s) { return ((((unsigned)x * kTchMul) >> (28 - LB)) & kMask) ^ s; }
  static __device__ __forceinline__ unsigned salt(int local_row) { return (((unsigned)local_row * 37u) & (unsigned)(STAGE - 1)) << 4; }
  static __device__ __forceinline__ int row_of(unsigned s) { return (int)(((s >> 4) * 941u) & (unsigned)(STAGE - 1)); }  // 37 * 941 = 1 mod 2048
};

__device__ __forceinline__ int tch_local_row(const int *rpl, const int nvl, const int e) {  // largest i with rpl[i] <= e
  int lo = 0, hi = nvl - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rpl[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Which of the T keys of this lane are in the row their salt names?  Lane masks throughout (see hrow_probe, gm_hrow.hip):
// hm = lanes whose key was found, nm = lanes that missed in a bucket that overflowed.
template <int STAGE, int T>
__device__ __forceinline__ void tch_probe(const TchLds<STAGE> &B, const int *__restrict__ col, const bool fallback, const int (&key)[T],
                                          const unsigned (&salt)[T], const unsigned long long (&inm)[T], unsigned long long (&hm)[T],
                                          unsigned long long (&nm)[T]) {
  if (fallback) {  // wave-uniform
#pragma unroll
    for (int q = 0; q < T; ++q) {
      bool f = false;
      if (__builtin_amdgcn_inverse_ballot_w64(inm[q])) {
        const int lo = TchHash<STAGE>::row_of(salt[q]);
        const int rs = B.rpl[lo], rn = B.rpl[lo + 1] - rs;
        const int pos = lower_bound(col + rs, rn, key[q]);
        f = pos < rn && col[rs + pos] == key[q];
      }
      hm[q] = __ballot(f);
      nm[q] = 0ull;
    }
    return;
  }
  uint4 w[T];
#pragma unroll
  for (int q = 0; q < T; ++q)
    w[q] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(B.table) + TchHash<STAGE>::bucket(key[q], salt[q]));
#pragma unroll
  for (int q = 0; q < T; ++q) {
    const unsigned k = (unsigned)key[q];
    const unsigned long long m = __ballot(w[q].x == k) | __ballot(w[q].y == k) | __ballot(w[q].z == k) | __ballot(w[q].w == k);
    hm[q] = m & inm[q];
    nm[q] = __ballot(w[q].w == kTchMarker) & ~m & inm[q];
  }
}

// The surplus list (<= 128 (id, salt) pairs, unused entries -1) is spread over the lanes, two entries each; a key that needs it is
// broadcast and compared by all lanes at once.  Returns the number of keys found.
template <int STAGE, int T>
__device__ __forceinline__ unsigned tch_surplus(const TchLds<STAGE> &B, const int lane, const int (&key)[T], const unsigned (&salt)[T],
                                                const unsigned long long (&nm)[T]) {
  const int k0 = B.ovf_key[lane], k1 = B.ovf_key[lane + GM_WAVE];
  const int s0 = B.ovf_salt[lane], s1 = B.ovf_salt[lane + GM_WAVE];
  unsigned c = 0;
#pragma unroll
  for (int q = 0; q < T; ++q) {
    unsigned long long rest = nm[q];
    while (rest) {
      const int src = __ffsll((long long)rest) - 1;
      rest &= rest - 1;
      const int k = readlane(key[q], src), s = readlane((int)salt[q], src);
      if (__ballot(((k0 == k) & (s0 == s)) | ((k1 == k) & (s1 == s))) != 0ull) ++c;
    }
  }
  return c;
}

// One batch of tasks: stream the lists (llen_all keys from col[key_base ..), 0 = no task) against the set; returns the matches (wave-uniform).
template <int STAGE, bool WIDE>
__device__ __forceinline__ unsigned tch_pass(TchLds<STAGE> &B, TchWave<TchLds<STAGE>::kBitWindow> &L, const int *__restrict__ col, const bool fallback, const int lane,
                                             const int llen_all, const int key_base, const unsigned salt_l) {
  // (tiles per group of a long list: a list of 200 .. 300 keys fills groups of 128 keys better than groups of 256 -- R-MAT-22, 1 / 2 / 3 / 4 tiles:
  // 3.14 / 2.89 / 3.02 / 3.03 ms; the 2048-bucket kernel streams longer lists: R-MAT-24 60.3 / 43.1 / 41.6 / 41.0)
  constexpr int T = STAGE <= 1024 ? kTchTilesSmall : kTchTiles;
  constexpr int TF = STAGE <= 1024 ? kTchFlatTilesSmall : kTchFlatTilesBig;
  unsigned cnt = 0;
  if (wave_max_nonneg(llen_all) == 0) return 0u;  // wave-uniform
  const bool is_long = llen_all >= kTchLongList;
  const int llen = is_long ? 0 : llen_all;

  // ---- long lists: one task at a time, wave-uniform base / salt; the keys of the NEXT tile group are requested before the current
  // group is looked up (unconditional, unclamped loads in the steady state: flat_pass_filtered, gm_flat.h) -----------------------------
  unsigned long long lm = __ballot(is_long);
  while (lm) {
    const int src = __ffsll((long long)lm) - 1;
    lm &= lm - 1;
    const int base = readlane(key_base, src);
    const int n = readlane(llen_all, src);
    const unsigned s_u = (unsigned)readlane((int)salt_l, src);
    const int *__restrict__ kp = col + base;
    // the first K tiles of a group (K = T in the steady state; the last group of a list looks up only the tiles it has)
    auto process = [&](auto kc, const int (&key)[T], const unsigned long long (&inm)[T]) {
      constexpr int K = decltype(kc)::value;
      int k2[K];
      unsigned salt[K];
      unsigned long long i2[K], hm[K], nm[K];
#pragma unroll
      for (int q = 0; q < K; ++q) {
        k2[q] = key[q];
        salt[q] = s_u;
        i2[q] = inm[q];
      }
      tch_probe<STAGE, K>(B, col, fallback, k2, salt, i2, hm, nm);
      unsigned long long any_need = 0ull;
#pragma unroll
      for (int q = 0; q < K; ++q) {
        cnt += (unsigned)__popcll(hm[q]);
        any_need |= nm[q];
      }
      if (any_need != 0ull) cnt += tch_surplus<STAGE, K>(B, lane, k2, salt, nm);  // rare
    };
    constexpr int G = GM_WAVE * T;
    int nxt[T];
#pragma unroll
    for (int q = 0; q < T; ++q) nxt[q] = kp[min(q * GM_WAVE + lane, n - 1)];
    int t = 0;
    for (; t + 2 * G <= n; t += G) {
      int key[T];
      unsigned long long inm[T];
#pragma unroll
      for (int q = 0; q < T; ++q) {
        key[q] = nxt[q];
        inm[q] = ~0ull;
      }
      const int *__restrict__ kn = kp + (t + G);
#pragma unroll
      for (int q = 0; q < T; ++q) nxt[q] = kn[(unsigned)(q * GM_WAVE + lane)];
      process(std::integral_constant<int, T>{}, key, inm);
    }
    for (; t < n; t += G) {
      int key[T];
      unsigned long long inm[T];
#pragma unroll
      for (int q = 0; q < T; ++q) {
        key[q] = nxt[q];
        inm[q] = __ballot((t + q * GM_WAVE + lane) < n);
      }
#pragma unroll
      for (int q = 0; q < T; ++q) nxt[q] = kp[min(t + G + q * GM_WAVE + lane, n - 1)];
      const int tiles = min(T, (n - t + GM_WAVE - 1) >> 6);  // wave-uniform
      if (tiles >= T) process(std::integral_constant<int, T>{}, key, inm);
      else if (tiles == 1) process(std::integral_constant<int, 1>{}, key, inm);
      else if constexpr (T > 2) {
        if (tiles == 2) process(std::integral_constant<int, 2>{}, key, inm);
        else process(std::integral_constant<int, (T > 2 ? 3 : 1)>{}, key, inm);
      }
    }
  }

  // ---- short lists: flattened.  Position p of the concatenated lists belongs to the LAST list that starts at or before it: every
  // list but the first of a window leaves one mark BIT at (its start - 1), and the owner of p is the number of marks below p -- one
  // broadcast 8-byte LDS read and a v_mbcnt pair per tile, a scalar popcount for the carry; a window is 8192 positions (1 KB of
  // marks), so that -- unlike the 512 byte-marks per window of the other kernels -- a whole batch is usually ONE window and the keys
  // of the NEXT tile group are requested before the current group is looked up (measured: TF = 8 tiles in flight without the
  // pipeline R-MAT-22 3.34 -> 3.22 ms).  On R-MAT-22 88 % of the streamed keys outside the hub corner pass through this loop and none
  // through the one-at-a-time path above, so its steady state is peeled: per 64 keys 8 vector instructions of lookup,
  // 5 of owner resolution, 1 of addressing (profiles/r13/ab_tc_flat_steady.txt) ------------------------------------------------------
  const int incl = wave_incl_scan_add(llen);
  const int total = readlane(incl, GM_WAVE - 1);
  if (total == 0) return cnt;  // wave-uniform
  const int off = incl - llen;
  const unsigned long long nzm = __ballot(llen > 0);
  // (compacted: the k-th non-empty list.  The narrow form keeps the key base as a BYTE offset modulo 2^32: see kTchFlatBias)
  if (llen > 0) L.desc[rank_below(nzm)] = make_int2(WIDE ? key_base - off : (int)((unsigned)(key_base - off) << 2), (int)salt_l);
  constexpr int G = GM_WAVE * TF, kBitWin = TchLds<STAGE>::kBitWindow;
  constexpr int TH = 4, NH = TF / TH;  // a group is looked up in halves of four tiles (the 16-byte buckets of eight would not fit the registers)
  static_assert(TF % TH == 0, "tile groups are made of half-groups of four");
  static_assert(kTchFlatBias >= 4u * (unsigned)(GM_WAVE * (kTchLongList - 1) + G), "the bias covers every flattened position of a batch and the over-run of its last group");
  struct Grp {
    int key[NH][TH];
    unsigned salt[NH][TH];
    unsigned long long inm[NH][TH];
  };
  // (the descriptors through their LDS byte address, wave-uniform: owner k is at dbase + 8 k, one shift-add from the v_mbcnt pair)
  using LdsDesc = const __attribute__((address_space(3))) unsigned long long;
  const unsigned dbase = (unsigned)readfirst((int)(unsigned)(size_t)(LdsDesc *)reinterpret_cast<const unsigned long long *>(&L.desc[0]));
  const char *const colb = reinterpret_cast<const char *>(col) - kTchFlatBias;  // (never dereferenced below col: every offset carries the bias)
  const unsigned lane4 = ((unsigned)lane << 2) + kTchFlatBias;  // (the bias rides on the lane's part of the offset)
  for (int wb = 0; wb < total; wb += kBitWin) {
    const int wn = min(kBitWin, total - wb);
    const int nw = ((wn + G - 1) / G) * (G / 32) + 2;
    for (int i = lane; i < nw; i += GM_WAVE) L.bits[i] = 0u;
    wave_sync();
    if (llen > 0 && off > wb && off < wb + kBitWin) atomicOr(&L.bits[(off - 1 - wb) >> 5], 1u << ((off - 1 - wb) & 31));
    // the descriptor of the list that owns position wb, as its LDS address; every mark passed moves it on by one descriptor
    unsigned carry = dbase + ((unsigned)(__popcll(__ballot(llen > 0 && off <= wb)) - 1) << 3);
    wave_sync();
    // owners, descriptors, key loads of tile group g of the window.  FULL: the group lies wholly inside the window and below `total`
    // (every group of a window but its last): no range test, no ballot, no guarded select on the owner and on the index.
    auto stage_a = [&](auto full, const int g, Grp &r) {
      constexpr bool FULL = decltype(full)::value;
      int2 d[TF];
      bool in[TF];
      const int p0 = wb + g * G;  // wave-uniform
      // the 2 * TF mark words of the group: one LDS read (lane l holds word l), then two v_readlane per tile
      const int mw = (int)L.bits[((g * G) >> 5) + (lane & (2 * TF - 1))];
#pragma unroll
      for (int q = 0; q < TF; ++q) {
        const unsigned long long m = ((unsigned long long)(unsigned)readlane(mw, 2 * q + 1) << 32) | (unsigned)readlane(mw, 2 * q);
        const unsigned own = carry + ((unsigned)rank_below(m) << 3);
        carry += (unsigned)__popcll(m) << 3;
        asm volatile("" : "+s"(carry));  // (kept in a scalar register as it stands: re-associated, every tile paid a vector add for its part of the sum)
        in[q] = FULL || (p0 + q * GM_WAVE + lane) < total;
        r.inm[q / TH][q % TH] = FULL ? ~0ull : __ballot(in[q]);
        const unsigned long long dw = *(LdsDesc *)(size_t)(in[q] ? own : dbase);  // unconditional LDS read, the descriptor as one 8-byte word
        d[q] = make_int2((int)(unsigned)dw, (int)(unsigned)(dw >> 32));
      }
#pragma unroll
      for (int q = 0; q < TF; ++q) {
        if constexpr (WIDE) {  // exact for every index below 2^31: the index as an unsigned 32-bit sum (d.x may be negative, the sum is not)
          const unsigned idx = (unsigned)d[q].x + (unsigned)(p0 + q * GM_WAVE + lane);
          r.key[q / TH][q % TH] = col[in[q] ? idx : 0u];  // unconditional load (select on the index)
        } else {
          // address = (col - bias + 4 p0) + zero-extended 32-bit (4 (key_base - off) + (4 lane + bias)) + 256 q: a scalar base, ONE
          // vector add, the tile in the load's immediate offset.  The 32-bit sum is 4 (index - p0 - 64 q) + bias with index - p0 - 64 q
          // > -(positions of a batch): never negative, and below 2^32 while the array streamed from has fewer than kTchNarrowEntries entries (gm_tch_rule.h).
          const unsigned idle = kTchFlatBias - ((unsigned)(p0 + q * GM_WAVE) << 2);  // a lane beyond `total` loads col[0]
          const unsigned voff = in[q] ? (unsigned)d[q].x + lane4 : idle;
          r.key[q / TH][q % TH] = *reinterpret_cast<const int *>(colb + ((size_t)(unsigned)p0 << 2) + (size_t)voff + (size_t)(q * GM_WAVE * 4));
        }
        r.salt[q / TH][q % TH] = (unsigned)d[q].y;
      }
    };
    auto stage_b = [&](auto full, const Grp &r) {
      constexpr bool FULL = decltype(full)::value;
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        unsigned long long inm[TH], hm[TH], nm[TH];
#pragma unroll
        for (int q = 0; q < TH; ++q) inm[q] = FULL ? ~0ull : r.inm[h][q];  // (a compile-time all-ones: no s_and on the hit and marker masks)
        tch_probe<STAGE, TH>(B, col, fallback, r.key[h], r.salt[h], inm, hm, nm);
        unsigned long long any_need = 0ull;
#pragma unroll
        for (int q = 0; q < TH; ++q) {
          cnt += (unsigned)__popcll(hm[q]);
          any_need |= nm[q];
        }
        if (any_need != 0ull) cnt += tch_surplus<STAGE, TH>(B, lane, r.key[h], r.salt[h], nm);  // rare
      }
    };
    // the full groups in the peeled form, one group ahead in flight; the last group of the window, if it is partial, in the guarded
    // form -- requested under the last full group's lookup, so the pipeline holds across the switch
    constexpr std::true_type kFull{};
    constexpr std::false_type kGuarded{};
    const int nfull = wn / G, ng = (wn + G - 1) / G;
    Grp cur;
    if (nfull == 0) {  // (wn > 0: the window is one partial group)
      stage_a(kGuarded, 0, cur);
    } else {
      stage_a(kFull, 0, cur);
      for (int g = 0; g + 1 < nfull; ++g) {
        Grp nxt;
        stage_a(kFull, g + 1, nxt);
        stage_b(kFull, cur);
        cur = nxt;
      }
      if (ng > nfull) {
        Grp nxt;
        stage_a(kGuarded, nfull, nxt);
        stage_b(kFull, cur);
        cur = nxt;
      }
    }
    stage_b(kGuarded, cur);  // (the last group, full or not: a full one carries all-ones masks)
    wave_sync();
  }
  return cnt;
}

#ifndef GM_TCH_MIN_WG
#define GM_TCH_MIN_WG 6
#endif
template <int STAGE, bool WIDE>
__global__ __launch_bounds__((tch_waves<STAGE>() * GM_WAVE), (STAGE <= 1024 ? GM_TCH_MIN_WG : GM_TCH_MIN_WG_BIG))
void tch_kernel(const MineParams p) {
  __shared__ TchLds<STAGE> B;
  using H = TchHash<STAGE>;
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const int wave = threadIdx.x >> 6;
  constexpr int nthreads = tch_waves<STAGE>() * GM_WAVE;
  const int tid = threadIdx.x;
  const int *__restrict__ rp = p.g.rp;
  const int *__restrict__ col = p.g.col;
  const int *__restrict__ trp = p.g.trp;
  const int2 *__restrict__ tdesc = p.g.tdesc;
  auto &L = B.w[wave];
  unsigned long long c0 = 0;  // wave-uniform
  for (;;) {
    if (tid == 0) B.queue_pos = atomicAdd(p.queue, (unsigned)p.grab);
    __syncthreads();
    const unsigned q = B.queue_pos;
    if (q >= (unsigned)p.count) break;
    const unsigned qe = min(q + (unsigned)p.grab, (unsigned)p.count);
    // The NEXT chunk of the dequeue is requested while the current one streams: its record, then (two dependent round trips that used to
    // sit between two chunks, with every wave of the workgroup waiting) its first kU * nthreads row entries and its offsets.
    constexpr int kU = 4;  // entries requested together per thread
    auto chunk_at = [&](const unsigned ci) {
      const size_t pos = (size_t)p.first + (size_t)ci * (size_t)p.step;
      return p.chunks[p.order ? (size_t)p.order[pos] : pos];
    };
    ChunkRec rn = chunk_at(q);
    bool have_pre = false;
    int xn[kU], rpn = 0, trpn = 0;
    for (unsigned ci = q; ci < qe; ++ci) {
      const ChunkRec r = rn;
      const int ub = r.u_begin, nvl = r.u_end - r.u_begin;
      const int eb = r.e_begin, nel = r.e_end - r.e_begin;
      // ---- workgroup: the chunk's DAG rows into the set -----------------------------------------------------------------
      unsigned *fill32 = reinterpret_cast<unsigned *>(&B.w[0]);
      if (have_pre) {  // (requested during the previous chunk; rows beyond 256 threads' reach: below)
        if (tid <= nvl) {
          B.rpl[tid] = rpn;
          B.trpl[tid] = trpn;
        }
        for (int i = tid + nthreads; i <= nvl; i += nthreads) {
          B.rpl[i] = rp[ub + i];
          B.trpl[i] = trp[ub + i];
        }
      } else {
        for (int i = tid; i <= nvl; i += nthreads) {
          B.rpl[i] = rp[ub + i];
          B.trpl[i] = trp[ub + i];
        }
      }
      {
        // (the two constants are made here, per chunk: hoisted out of the dequeue loop, their register tuples -- four words of ones,
        // two of zeros -- stayed occupied across the streaming loops, which have none to spare at six waves per SIMD)
        unsigned ones = kTchEmpty, zero = 0u;
        asm volatile("" : "+v"(ones), "+v"(zero));
        const uint4 empty = make_uint4(ones, ones, ones, ones);
        for (int i = tid; i < STAGE; i += nthreads) B.table[i] = empty;
        for (int i = tid; i < STAGE / 2; i += nthreads) fill32[i] = zero;
        if (tid < kTchOvfCap) {
          B.ovf_key[tid] = (int)ones;
          B.ovf_salt[tid] = (int)ones;
        }
        if (tid == 0) {
          B.n_ovf = (int)zero;
          B.next_batch = (int)zero;
          B.next_group = (int)zero;
        }
      }
      __syncthreads();
      unsigned *slots = reinterpret_cast<unsigned *>(B.table);
      for (int i0 = tid; i0 < nel; i0 += kU * nthreads) {
        int x[kU];
        if (have_pre && i0 == tid) {
#pragma unroll
          for (int j = 0; j < kU; ++j) x[j] = xn[j];
        } else {
#pragma unroll
          for (int j = 0; j < kU; ++j) x[j] = col[eb + min(i0 + j * nthreads, nel - 1)];
        }
#pragma unroll
        for (int j = 0; j < kU; ++j) {
          const int i = i0 + j * nthreads;
          if (i < nel) {
            const unsigned s = H::salt(tch_local_row(B.rpl, nvl, eb + i));
            const unsigned b = H::bucket(x[j], s) >> 4;
            const unsigned shift = (b & 1u) * 16u;
            const unsigned slot = (atomicAdd(&fill32[b >> 1], 1u << shift) >> shift) & 0xffffu;
            if (slot < 4u) {
              slots[(b << 2) + slot] = (unsigned)x[j];
            } else {
              const int jo = atomicAdd(&B.n_ovf, 1);
              if (jo < kTchOvfCap) {
                B.ovf_key[jo] = x[j];
                B.ovf_salt[jo] = (int)s;
              }
            }
          }
        }
      }
      __syncthreads();
      // a bucket that got more than four entries gives up its last slot for the marker; the entry that sat there joins the surplus
      // list -- its salt comes back from (bucket, id): bucket = hash(id) ^ salt
      for (int b = tid; b < STAGE; b += nthreads) {
        const unsigned c = (fill32[b >> 1] >> ((b & 1) * 16)) & 0xffffu;
        if (c > 4u) {
          const unsigned x3 = slots[(b << 2) + 3];
          const int jo = atomicAdd(&B.n_ovf, 1);
          if (jo < kTchOvfCap) {
            B.ovf_key[jo] = (int)x3;
            B.ovf_salt[jo] = (int)(H::bucket((int)x3, 0u) ^ ((unsigned)b << 4));
          }
          slots[(b << 2) + 3] = kTchMarker;
        }
      }
      __syncthreads();  // (also: the fill counters are dead, the waves may use their scratch)
      const bool fallback = B.n_ovf > kTchOvfCap || (p.flags & (1 << 22)) != 0;
      have_pre = ci + 1 < qe;  // (workgroup-uniform)
      if (have_pre) {
        rn = chunk_at(ci + 1);
        const int nel_n = rn.e_end - rn.e_begin, nvl_n = rn.u_end - rn.u_begin;
#pragma unroll
        for (int j = 0; j < kU; ++j) xn[j] = col[rn.e_begin + min(tid + j * nthreads, max(nel_n - 1, 0))];
        rpn = rp[rn.u_begin + min(tid, nvl_n)];
        trpn = trp[rn.u_begin + min(tid, nvl_n)];
      }
      // ---- waves: the KEY STREAM of the chunk's short lists (GraphView::kst) -- the keys of every list of <= GM_TC_INLINE_MAX entries
      // its vertices host, in task order, each tagged with the low 8 bits of its host: one contiguous range per chunk, one coalesced
      // load per 64 keys, no descriptor, no row search, no flattening (a task of LiveJournal's shape -- nine keys -- cost a random
      // 64-byte line or two and its share of the batch bookkeeping); the next group's keys are requested before the current one is
      // looked up.  Parts of a heavy chunk interleave the groups like they interleave the batches below.
      if (p.g.kst != nullptr) {
        constexpr int TS = 4, GS = TS * GM_WAVE;
        const int kb = p.g.kst_rp[ub], kn = p.g.kst_rp[ub + nvl] - kb;
        const unsigned *__restrict__ kp = p.g.kst + kb;
        auto grab = [&]() {
          int gi = 0;
          if (lane == 0) gi = atomicAdd(&B.next_group, 1);
          return (readfirst(gi) * r.nparts + r.part) * GS;
        };
        unsigned nxt[TS];
        int g0 = kn > 0 ? grab() : 0;
        if (g0 < kn) {
#pragma unroll
          for (int q = 0; q < TS; ++q) nxt[q] = kp[min(g0 + q * GM_WAVE + lane, kn - 1)];
        }
        while (g0 < kn) {  // wave-uniform
          const int gc = g0;
          int key[TS];
          unsigned salt[TS];
          unsigned long long inm[TS], hm[TS], nm[TS];
#pragma unroll
          for (int q = 0; q < TS; ++q) {
            key[q] = (int)(nxt[q] & 0xffffffu);
            salt[q] = H::salt((int)(((nxt[q] >> 24) - (unsigned)ub) & 255u));  // host = ub + local row, local row < 256
            inm[q] = __ballot(gc + q * GM_WAVE + lane < kn);
          }
          g0 = grab();
          if (g0 < kn) {
#pragma unroll
            for (int q = 0; q < TS; ++q) nxt[q] = kp[min(g0 + q * GM_WAVE + lane, kn - 1)];
          }
          tch_probe<STAGE, TS>(B, col, fallback, key, salt, inm, hm, nm);
          unsigned long long any_need = 0ull;
          unsigned cnt = 0;
#pragma unroll
          for (int q = 0; q < TS; ++q) {
            cnt += (unsigned)__popcll(hm[q]);
            any_need |= nm[q];
          }
          if (any_need != 0ull) cnt += tch_surplus<STAGE, TS>(B, lane, key, salt, nm);  // rare
          c0 += (unsigned long long)cnt;
        }
      }
      // ---- waves: batches of 64 tasks ---------------------------------------------------------------------------------
      const int tb = readfirst(B.trpl[0]), ntask = readfirst(B.trpl[nvl]) - tb;  // (scalar registers: they live across every batch)
      for (;;) {
        int bi = 0;
        if (lane == 0) bi = atomicAdd(&B.next_batch, 1);
        bi = readfirst(bi) * r.nparts + r.part;
        const int t0 = bi * GM_WAVE;
        if (t0 >= ntask) break;
        const bool valid = t0 + lane < ntask;
        const int te = tb + min(t0 + lane, ntask - 1);
        const int2 d = tdesc[te];                       // {start, length} of the list to stream, coalesced
        const int lo = tch_local_row(B.trpl, nvl, te);  // the host row of this task
        const int ru = B.rpl[lo], a = B.rpl[lo + 1] - ru;
        const bool act = valid && d.y > 0 && a > 0;
        c0 += (unsigned long long)tch_pass<STAGE, WIDE>(B, L, col, fallback, lane, act ? d.y : 0, d.x, H::salt(lo));
      }
      __syncthreads();  // the table is rewritten by the next chunk
    }
  }
  if (lane == 0 && c0) atomicAdd(&p.counters[0], c0);
}

// 1024 buckets (16 KB of LDS + 7.6 KB: six workgroups per CU) or 2048 (32 KB: four) -- the longest DAG row must fit
int tch_per_cu(int stage) {
  if (stage <= 1024) return 6;
  return (int)std::max<size_t>(1, std::min<size_t>(163840 / sizeof(TchLds<kTctStageMax>), 2048 / (tch_waves<kTctStageMax>() * GM_WAVE)));
}
hipError_t launch_tch(const MineParams &p, int stage, int grid_blocks, hipStream_t stream) {
  static_assert(sizeof(TchLds<1024>) * 6 <= 163840, "six workgroups per CU");
  static_assert(sizeof(TchLds<kTctStageMax>) <= 163840, "one workgroup per CU at least");
  static_assert(sizeof(TchWave<4096>) * tch_waves<kTctStageMax>() >= (size_t)kTctStageMax * 2, "fill counters alias the wave scratch");
  if (p.g.trp == nullptr || p.g.tdesc == nullptr) return hipErrorInvalidValue;
  const dim3 grid((unsigned)grid_blocks);
  // (the rule of gm_tch_rule.h, on the extent of the array the keys are streamed from -- not on the DAG's own entry count)
  const bool wide = tch_wide_form(tch_key_entries(p.g.ne, p.g.col_entries), gm_opt("GM_TCH_WIDE_NE"));
  const dim3 block_small(kWavesPerBlock * GM_WAVE), block_big(tch_waves<kTctStageMax>() * GM_WAVE);
  if (stage <= 1024) {
    if (wide) hipLaunchKernelGGL((tch_kernel<1024, true>), grid, block_small, 0, stream, p);
    else hipLaunchKernelGGL((tch_kernel<1024, false>), grid, block_small, 0, stream, p);
  } else {
    if (wide) hipLaunchKernelGGL((tch_kernel<kTctStageMax, true>), grid, block_big, 0, stream, p);
    else hipLaunchKernelGGL((tch_kernel<kTctStageMax, false>), grid, block_big, 0, stream, p);
  }
  return hipGetLastError();
}

}  // namespace gm

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_tch_kernel() {}
void gm_touch_tch() { hipLaunchKernelGGL(gm_touch_tch_kernel, dim3(1), dim3(1), 0, 0); }
