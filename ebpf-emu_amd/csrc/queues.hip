// queues.hip — what a datapath does with a batch's verdicts: the stable
// partition of the packet numbers by XDP action (ebpf_verdict_queues) and the copy of one queue's
// packets into a dense offsets + lens batch (ebpf_gather), and the way back (§3.39): that dense
// batch's packets and results put back at the packets' own numbers (ebpf_scatter, one launch);
// and the way out (§3.40): one queue written as a classic libpcap byte stream (ebpf_pcap_gather).
// New: no reference counterpart (the reference runs one packet and prints r0); xdp.rs:3-9 is the
// action enum the queues follow.
//
// The queues and the two gathers are count -> bases -> write over contiguous per-workgroup ranges,
// in separate launches: the launch boundary is the only ordering between workgroups. No workgroup
// ever waits on another one's progress (no look-back, no flag, no grid barrier, no cooperative
// launch), so a grid larger than the resident set cannot hang. No device atomics; the only LDS
// atomics add up sums whose order does not matter.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"

namespace ebpfemu {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// (any address: a clang vector, not HIP_vector_type, whose 16-byte aligned copy constructor would
// be handed the 1-byte aligned lvalue)
typedef uint32_t u32x4_any __attribute__((ext_vector_type(4), aligned(1)));
typedef __attribute__((address_space(1))) const u32x4 g_u4;
typedef __attribute__((address_space(1))) const u32x4_any g_u4_any;
typedef __attribute__((address_space(1))) const uint32_t g_u32;
typedef uint64_t u64_any __attribute__((aligned(1)));
typedef uint32_t u32_any __attribute__((aligned(1)));
typedef uint16_t u16_any __attribute__((aligned(1)));

__device__ __forceinline__ uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// ============================================================================================
// Verdict queues. Workgroup g owns the packets [g * S, (g + 1) * S), S a whole number of kQRange
// (one while the grid is not capped); wave w of it the w-th quarter, walked 256 packets a step:
// one dword of four verdicts per lane, then four sub-steps of 64 packets with lane = packet, so
// the packet order is (workgroup, wave, step, lane) and a class's index stores are consecutive.
// ============================================================================================
__device__ __forceinline__ uint32_t q_class(uint32_t v) { return v < 5 ? v : v == 0xFFu ? 6u : 5u; }

struct QSpan {
  uint64_t beg, end;
};
__device__ __forceinline__ QSpan q_wave_span(uint64_t n, uint32_t grid, uint32_t g, uint32_t w) {
  const uint64_t per = (n + grid - 1) / grid;
  const uint64_t S = (per + kQRange - 1) / kQRange * kQRange;
  const uint64_t q = S / kQWaves;  // a multiple of 256
  QSpan s;
  s.beg = (uint64_t)g * S + (uint64_t)w * q;
  s.end = s.beg + q;
  if (s.beg > n) s.beg = n;
  if (s.end > n) s.end = n;
  return s;
}

// The verdict bytes [e + 4 lane, e + 4 lane + 4) as one dword, at any alignment of `v`: the two
// aligned dwords that hold them (each read only where it holds a byte of v[0, n)), funnel-shifted.
// Bytes at or past n are unspecified.
__device__ __forceinline__ uint32_t q_load4(const uint8_t* v, uint64_t n, uint64_t e, uint32_t lane) {
  const uintptr_t p0 = (uintptr_t)v, pend = p0 + n;
  const uintptr_t p = p0 + e + 4 * lane;
  const uintptr_t a = p & ~(uintptr_t)3;
  const uint32_t sh = (uint32_t)(p & 3);
  const uint32_t lo = a < pend ? *(g_u32*)a : 0u;  // (a + 4 > p >= p0)
  const uint32_t hi = (sh && a + 4 < pend) ? *(g_u32*)(a + 4) : 0u;
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

// Class of packet e + 64 j + lane from the step's dwords (7: past the wave's range).
__device__ __forceinline__ uint32_t q_step_class(uint32_t dw, uint32_t j, uint32_t lane, uint64_t i,
                                                 uint64_t end) {
  const uint32_t d = (uint32_t)__shfl((int)dw, (int)(16 * j + (lane >> 2)));
  return i < end ? q_class((d >> (8 * (lane & 3))) & 0xFFu) : 7u;
}

// Per-wave class counts (wvc[g][w][8]) and their workgroup sums (wgc[g][8]), plain stores.
__global__ __launch_bounds__(kQBlock) void queues_count(const uint8_t* __restrict__ verdict,
                                                        uint64_t n, uint32_t* __restrict__ wgc,
                                                        uint32_t* __restrict__ wvc) {
  __shared__ uint32_t s[kQWaves][kQSlots];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6, g = blockIdx.x;
  const QSpan sp = q_wave_span(n, gridDim.x, g, w);
  uint32_t cnt[kQClasses] = {0, 0, 0, 0, 0, 0, 0};
  for (uint64_t e = sp.beg; e < sp.end; e += 256) {
    const uint32_t dw = q_load4(verdict, n, e, lane);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      const uint32_t c = q_step_class(dw, j, lane, e + 64 * j + lane, sp.end);
#pragma unroll
      for (uint32_t q = 0; q < (uint32_t)kQClasses; q++) cnt[q] += (uint32_t)__popcll(ballot(c == q));
    }
  }
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t q = 0; q < (uint32_t)kQClasses; q++) mine = lane == q ? cnt[q] : mine;
  if (lane < (uint32_t)kQSlots) {
    s[w][lane] = mine;
    wvc[((uint64_t)g * kQWaves + w) * kQSlots + lane] = mine;
  }
  __syncthreads();
  if (t < (uint32_t)kQSlots) {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kQWaves; k++) sum += s[k][t];
    wgc[(uint64_t)g * kQSlots + t] = sum;
  }
}

// Each workgroup sums the class totals and the counts of the workgroups before it (as bin_scatter
// does), prefix-sums its waves' counts in LDS in wave order, then every wave writes its packets'
// numbers from base(class) = packets of lower classes + earlier workgroups' + earlier waves' of
// the class, a lane's rank inside its class from the class's ballot and the lanes below it.
__global__ __launch_bounds__(kQBlock) void queues_scatter(const uint8_t* __restrict__ verdict,
                                                          uint64_t n, const uint32_t* __restrict__ wgc,
                                                          const uint32_t* __restrict__ wvc,
                                                          uint32_t* __restrict__ index,
                                                          uint32_t* __restrict__ count) {
  static_assert(kQBlock % kQSlots == 0, "class of a thread fixed across the sum");
  __shared__ uint32_t tot[kQSlots], pre[kQSlots], wv[kQWaves][kQSlots], base[kQWaves][kQSlots];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6, g = blockIdx.x;
  if (t < (uint32_t)kQSlots) tot[t] = pre[t] = 0;
  if (t < (uint32_t)(kQWaves * kQSlots))
    wv[t / kQSlots][t % kQSlots] = wvc[(uint64_t)g * kQWaves * kQSlots + t];
  __syncthreads();
  uint32_t my_tot = 0, my_pre = 0;
  for (uint32_t j = t; j < gridDim.x * (uint32_t)kQSlots; j += kQBlock) {
    const uint32_t v = wgc[j];
    my_tot += v;
    if (j / kQSlots < g) my_pre += v;
  }
  if (my_tot) atomicAdd(&tot[t % kQSlots], my_tot);  // (sums: their order does not matter)
  if (my_pre) atomicAdd(&pre[t % kQSlots], my_pre);
  __syncthreads();
  if (t < (uint32_t)(kQWaves * kQSlots)) {
    const uint32_t ww = t / kQSlots, q = t % kQSlots;
    uint32_t start = pre[q];
    for (uint32_t c = 0; c < q; c++) start += tot[c];
    for (uint32_t k = 0; k < ww; k++) start += wv[k][q];  // the cross-wave prefix, in wave order
    base[ww][q] = start;
  }
  if (g == 0 && t < (uint32_t)kQClasses) count[t] = tot[t];
  __syncthreads();
  uint32_t wb[kQClasses];
#pragma unroll
  for (uint32_t q = 0; q < (uint32_t)kQClasses; q++) wb[q] = base[w][q];
  const QSpan sp = q_wave_span(n, gridDim.x, g, w);
  const uint64_t below = (1ull << lane) - 1;
  for (uint64_t e = sp.beg; e < sp.end; e += 256) {
    const uint32_t dw = q_load4(verdict, n, e, lane);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      const uint64_t i = e + 64 * j + lane;
      const uint32_t c = q_step_class(dw, j, lane, i, sp.end);
      uint32_t pos = 0;
#pragma unroll
      for (uint32_t q = 0; q < (uint32_t)kQClasses; q++) {
        const uint64_t m = ballot(c == q);
        pos = c == q ? wb[q] + (uint32_t)__popcll(m & below) : pos;
        wb[q] += (uint32_t)__popcll(m);
      }
      if (c < (uint32_t)kQClasses) index[pos] = (uint32_t)i;
    }
  }
}

// ============================================================================================
// Gather. The queue's m = count[queue] packets (read on the device) are split into contiguous
// per-workgroup ranges of a whole number of kGTile positions; gather_sums adds up each range's
// alignup(len); gather_copy sums the ranges before its own into its output base, then walks its
// range a tile at a time: a thread per packet for the entries, then the tile's 16-byte source
// chunks dealt to the lanes as xdp_stage deals its (each wave a quarter of the tile's chunks, its
// lanes on consecutive chunks, each mapped to its packet through the chunk prefix sums in LDS).
// A chunk is 16 bytes of ONE packet at packet offset 16 c, stored at out_offsets[j] + 16 c: with
// align >= 16 these are the 16-byte chunks of the output range; with align < 16 an output chunk
// would straddle packets, so the chunks stay per packet and a packet's last, partial chunk is
// stored byte-exact.
// ============================================================================================
__device__ __forceinline__ u32x4 blk16(uintptr_t a, uintptr_t src, uintptr_t end) {
  if (a + 16 <= src || a >= end) return u32x4{0u, 0u, 0u, 0u};
  return *(g_u4*)a;
}

// Packet bytes [off, off + rem) of a packet of len bytes at src, 1 <= rem <= 15 and off + rem <=
// len (a partial chunk), in the result's low bytes: the two aligned 16-byte blocks that hold them,
// each read only where it holds a byte of the packet, funnel-shifted (v_alignbyte); the bytes at
// or past rem are zero.
__device__ __forceinline__ u32x4 span_load(const uint8_t* src, uint32_t len, uint32_t off,
                                           uint32_t rem) {
  const uintptr_t s0 = (uintptr_t)src, end = s0 + len;
  const uintptr_t p = s0 + off;
  const uintptr_t a0 = p & ~(uintptr_t)15;
  const uint32_t sh = (uint32_t)(p & 15), q = sh >> 2;
  const u32x4 b0 = blk16(a0, s0, end);
  const u32x4 b1 = sh ? blk16(a0 + 16, s0, end) : u32x4{0u, 0u, 0u, 0u};
  const uint32_t d[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    // d[k + q] and d[k + q + 1] by selects (q per thread: no dynamic register indexing)
    const uint32_t l0 = (q & 1) ? d[k + 1] : d[k], l1 = (q & 1) ? d[k + 3] : d[k + 2];
    const uint32_t h0 = (q & 1) ? d[k + 2] : d[k + 1];
    const uint32_t h1 = (q & 1) ? (k + 4 < 8 ? d[k + 4] : 0u) : d[k + 3];
    const uint32_t lo = (q & 2) ? l1 : l0, hi = (q & 2) ? h1 : h0;
    const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, sh & 3);
    const uint32_t valid = rem > 4u * k ? min(rem - 4u * k, 4u) : 0u;
    w[k] = valid >= 4 ? v : v & ((1u << (8 * valid)) - 1u);
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}

// A packet's last, partial chunk: its bytes [16 c, len), 16 c < len < 16 c + 16.
__device__ __forceinline__ u32x4 tail_chunk(const uint8_t* src, uint32_t len, uint32_t c) {
  return span_load(src, len, 16 * c, len - 16 * c);
}

// The first rem (1..15) bytes of v to dst, no byte more: 8 + 4 + 2 + 1.
__device__ __forceinline__ void store_bytes(uint8_t* dst, u32x4 v, uint32_t rem) {
  uint64_t lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
  const uint64_t hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
  if (rem & 8) {
    *(u64_any*)dst = lo;
    lo = hi;
    dst += 8;
  }
  if (rem & 4) {
    *(u32_any*)dst = (uint32_t)lo;
    lo >>= 32;
    dst += 4;
  }
  if (rem & 2) {
    *(u16_any*)dst = (uint16_t)lo;
    lo >>= 16;
    dst += 2;
  }
  if (rem & 1) *dst = (uint8_t)lo;
}

struct GQueue {
  uint32_t start, m;  // the queue is index[start .. start + m)
  uint64_t span;      // queue positions per workgroup
};
template <class Args>  // GatherArgs, PcapArgs: the queue under the same names
__device__ __forceinline__ GQueue g_queue(const Args& a, uint32_t grid) {
  uint64_t start = 0;
  for (uint32_t c = 0; c < a.queue; c++) start += a.count[c];
  uint64_t m = a.count[a.queue];
  // (counts that do not belong to this batch: stay inside index[0, n))
  if (start > a.n) start = a.n;
  if (m > a.n - start) m = a.n - start;
  GQueue q;
  q.start = (uint32_t)start;
  q.m = (uint32_t)m;
  const uint64_t per = (m + grid - 1) / grid;
  q.span = (per + kGTile - 1) / kGTile * kGTile;
  return q;
}

// Queue position j's packet: its bytes and length (a packet number outside the batch: no bytes).
__device__ __forceinline__ uint32_t g_packet(const GatherArgs& a, const GQueue& q, uint64_t j,
                                             const uint8_t** src) {
  const uint64_t i = a.index[q.start + j];
  *src = a.frames;
  if (i >= a.n) return 0u;
  *src = a.frames + (a.offsets ? (uint64_t)a.offsets[i] : i * a.stride);
  return a.lens ? (uint32_t)a.lens[i] : (uint32_t)a.stride;
}

__device__ __forceinline__ uint32_t g_alignup(uint32_t len, uint32_t align) {
  return (len + align - 1) & ~(align - 1);
}

// Sum over the workgroup (every thread gets it); red: u64[kGTile] in LDS.
__device__ __forceinline__ uint64_t block_sum(uint64_t v, unsigned long long* red, uint32_t t) {
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (uint32_t d = kGTile / 2; d > 0; d >>= 1) {
    if (t < d) red[t] += red[t + d];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kGTile) void gather_sums(GatherArgs a) {
  __shared__ unsigned long long red[kGTile];
  const uint32_t t = threadIdx.x, g = blockIdx.x;
  const GQueue q = g_queue(a, gridDim.x);
  const uint64_t beg = (uint64_t)g * q.span;
  const uint64_t end = beg + q.span < q.m ? beg + q.span : q.m;
  uint64_t sum = 0;
  for (uint64_t j = beg + t; j < end; j += kGTile) {
    const uint8_t* src;
    sum += g_alignup(g_packet(a, q, j, &src), a.align);
  }
  sum = block_sum(sum, red, t);
  if (t == 0) a.wsum[g] = sum;
}

__global__ __launch_bounds__(kGTile) void gather_copy(GatherArgs a) {
  __shared__ uint32_t pre[kGTile], cpre[kGTile], len_s[kGTile];
  __shared__ const uint8_t* src_s[kGTile];
  __shared__ unsigned long long red[kGTile];
  const uint32_t t = threadIdx.x, g = blockIdx.x;
  const GQueue q = g_queue(a, gridDim.x);
  if (q.m == 0) {
    if (g == 0 && t == 0) a.out_total[0] = a.out_total[1] = 0;
    return;
  }
  const uint64_t beg = (uint64_t)g * q.span;
  const uint64_t end = beg + q.span < q.m ? beg + q.span : q.m;
  if (beg >= end) return;  // (uniform)
  uint64_t B = 0;          // the output offset of the tile's first packet
  for (uint32_t k = t; k < g; k += kGTile) B += a.wsum[k];
  B = block_sum(B, red, t);
  for (uint64_t tb = beg; tb < end; tb += kGTile) {
    const uint64_t j = tb + t;
    const bool have = j < end;
    const uint8_t* src = a.frames;
    const uint32_t len = have ? g_packet(a, q, j, &src) : 0u;
    const uint32_t alen = have ? g_alignup(len, a.align) : 0u;
    pre[t] = alen;
    __syncthreads();
    for (uint32_t d = 1; d < kGTile; d <<= 1) {  // inclusive scan of the aligned lengths
      const uint32_t v = t >= d ? pre[t - d] : 0u;
      __syncthreads();
      pre[t] += v;
      __syncthreads();
    }
    const uint64_t off = B + pre[t] - alen;
    const bool wr = have && off + len <= a.cap;
    len_s[t] = have ? len : 0u;
    src_s[t] = src;
    cpre[t] = wr ? (len + 15) / 16 : 0u;
    __syncthreads();
    for (uint32_t d = 1; d < kGTile; d <<= 1) {  // inclusive scan of the chunk counts
      const uint32_t v = t >= d ? cpre[t - d] : 0u;
      __syncthreads();
      cpre[t] += v;
      __syncthreads();
    }
    if (wr) {
      a.out_offsets[j] = (uint32_t)off;
      a.out_lens[j] = (uint16_t)len;
      // the written packets are a prefix of the queue: the last one reports the totals
      bool next = false;
      if (j + 1 < q.m) {
        const uint8_t* s1;
        const uint32_t len1 = (t + 1 < kGTile && j + 1 < end) ? len_s[t + 1] : g_packet(a, q, j + 1, &s1);
        next = off + alen + len1 <= a.cap;
      }
      if (!next) {
        a.out_total[0] = (uint32_t)(j + 1);
        a.out_total[1] = (uint32_t)(off + len);
      }
    } else if (have && j == 0) {
      a.out_total[0] = a.out_total[1] = 0;
    }
    // wave w copies the w-th quarter of the tile's chunks, lane l the chunks l, l + 64, ... of it,
    // four in flight before any store (each chunk's packet: the first p with cpre[p] > k, found
    // by a binary search for the lane's first chunk, then walked forward)
    const uint32_t chunks = cpre[kGTile - 1];
    const uint32_t wv = t >> 6, ln = t & 63, qc = (chunks + 3) / 4;
    const uint32_t kb = min(wv * qc, chunks), ke = min(kb + qc, chunks);
    uint32_t p = 0;
    if (kb + ln < ke) {
      uint32_t lo = 0, hi = kGTile - 1;  // (cpre[kGTile - 1] > k for every k < chunks)
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cpre[mid] <= kb + ln) lo = mid + 1;
        else hi = mid;
      }
      p = lo;
    }
    for (uint32_t k0 = kb + ln; k0 < ke; k0 += 4 * 64) {
      u32x4 v[4];
      uint8_t* dst[4];
      uint32_t rem[4];  // 0: nothing, 16: the whole chunk, else that many bytes
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t k = k0 + 64 * u;
        rem[u] = 0;
        dst[u] = a.out_frames;
        v[u] = u32x4{0u, 0u, 0u, 0u};
        if (k >= ke) continue;
        while (cpre[p] <= k) p++;
        const uint32_t c = k - (p ? cpre[p - 1] : 0u);
        const uint32_t lp = len_s[p];
        const uint8_t* sp = src_s[p];
        const uint64_t o = B + pre[p] - g_alignup(lp, a.align) + 16ull * c;  // output offset
        dst[u] = a.out_frames + o;
        const uint32_t left = lp - 16 * c;
        if (left >= 16) {  // inside the packet: one load, as it lies
          const u32x4_any x = *(g_u4_any*)((uintptr_t)sp + 16ull * c);
          v[u] = u32x4{x.x, x.y, x.z, x.w};
          rem[u] = 16;
        } else {
          v[u] = tail_chunk(sp, lp, c);
          // the bytes past the packet's end are its padding only with align >= 16, and only below
          // out_bytes
          rem[u] = (a.align >= 16 && o + 16 <= a.cap) ? 16u : left;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (rem[u] == 16) *(u32x4_any*)dst[u] = v[u];
        else if (rem[u]) store_bytes(dst[u], v[u], rem[u]);
      }
    }
    B += pre[kGTile - 1];
    __syncthreads();  // (the next tile rewrites the LDS arrays)
  }
}

// ============================================================================================
// Pcap gather: the gather with a 16-byte record header in front of every packet
// and the 24-byte global header in front of all. The layout is the gather's at align 1 with
// 16 + incl in place of the length and a base of 24; a record is 1 + ceil(incl / 16) chunks at
// record offset 16 c -- chunk 0 the header (built in registers, or loaded from the 16 bytes before
// the packet), chunk c >= 1 the packet's bytes [16 (c - 1), ...), the last one stored byte-exact
// -- dealt to the lanes as gather_copy deals its. A packet number outside the batch is no record
// at all, so a record's number is not its queue position: pcap_sums also counts each range's
// records and notes the size of its first one, and the totals are reported by the one workgroup
// that can tell from those that its last written record is the last one (no atomics, no flags).
// ============================================================================================
struct PRec {
  uint32_t i;          // the source packet number (>= n: no record)
  uint32_t len, incl;  // its length, and the bytes of it the record holds
  const uint8_t* src;
};
__device__ __forceinline__ PRec p_record(const PcapArgs& a, const GQueue& q, uint64_t j) {
  PRec r;
  r.i = a.index[q.start + j];
  r.len = r.incl = 0;
  r.src = a.frames;
  if (r.i >= a.n) return r;  // (no address is formed from it)
  r.src = a.frames + (a.offsets ? (uint64_t)a.offsets[r.i] : r.i * a.stride);
  r.len = a.lens ? (uint32_t)a.lens[r.i] : (uint32_t)a.stride;
  r.incl = (a.snaplen && a.snaplen < r.len) ? a.snaplen : r.len;
  return r;
}

// Minimum over the workgroup (every thread gets it); red: u64[kGTile] in LDS.
__device__ __forceinline__ uint64_t block_min(uint64_t v, unsigned long long* red, uint32_t t) {
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (uint32_t d = kGTile / 2; d > 0; d >>= 1) {
    if (t < d && red[t + d] < red[t]) red[t] = red[t + d];
    __syncthreads();
  }
  return red[0];
}

// Inclusive scan of v[kGTile] (LDS) in place, v[t] written by thread t just before the call
// (gather_copy's scan steps).
__device__ __forceinline__ void tile_scan(uint32_t* v, uint32_t t) {
  __syncthreads();
  for (uint32_t d = 1; d < kGTile; d <<= 1) {
    const uint32_t x = t >= d ? v[t - d] : 0u;
    __syncthreads();
    v[t] += x;
    __syncthreads();
  }
}

// Per range: the bytes of its records, their number, and the bytes of the first one (0: none).
__global__ __launch_bounds__(kGTile) void pcap_sums(PcapArgs a) {
  __shared__ unsigned long long red[kGTile];
  const uint32_t t = threadIdx.x, g = blockIdx.x;
  const GQueue q = g_queue(a, gridDim.x);
  const uint64_t beg = (uint64_t)g * q.span;
  const uint64_t end = beg + q.span < q.m ? beg + q.span : q.m;
  uint64_t sum = 0, cnt = 0;
  uint64_t first = ~0ull;  // (position << 17 | record bytes) of the thread's first record
  for (uint64_t j = beg + t; j < end; j += kGTile) {
    const PRec r = p_record(a, q, j);
    if (r.i >= a.n) continue;
    sum += 16 + r.incl;
    cnt++;
    if (first == ~0ull) first = (j << 17) | (16 + r.incl);  // (j < 2^32, 16 + incl < 2^17)
  }
  sum = block_sum(sum, red, t);
  cnt = block_sum(cnt, red, t);
  first = block_min(first, red, t);
  if (t == 0) {
    a.wsum[g] = sum;
    a.wcnt[g] = (uint32_t)cnt;
    a.wfirst[g] = cnt ? (uint32_t)(first & 0x1FFFFu) : 0u;
  }
}

__global__ __launch_bounds__(kGTile) void pcap_copy(PcapArgs a) {
  // sc: (records written << kPShift | their chunks), scanned together: a tile has at most
  // 256 * (1 + 4096) chunks
  constexpr uint32_t kPShift = 22, kPMask = (1u << kPShift) - 1;
  static_assert(kGTile * (1u + 65536u / 16u) <= kPMask && kGTile < (1u << (32 - kPShift)), "sc");
  __shared__ uint32_t pre[kGTile], sc[kGTile], cpre[kGTile], len_s[kGTile], incl_s[kGTile], idx_s[kGTile];
  __shared__ const uint8_t* src_s[kGTile];
  __shared__ unsigned long long red[kGTile];
  __shared__ uint32_t last_end;  // the end byte of the range's last written record
  const uint32_t t = threadIdx.x, g = blockIdx.x, grid = gridDim.x;
  const bool swap = (a.flags & kPcapSwapped) != 0;
  if (g == 0 && t == 0) {  // the global header, and the totals when no record at all is written
    if (a.cap < 24) {
      a.out_total[0] = a.out_total[1] = 0;
    } else {
      *(u32x4_any*)a.out = u32x4{a.hdr[0], a.hdr[1], a.hdr[2], a.hdr[3]};
      *(u64_any*)(a.out + 16) = (uint64_t)a.hdr[4] | ((uint64_t)a.hdr[5] << 32);
      uint32_t k = 0;
      while (k < grid && a.wcnt[k] == 0) k++;
      if (k == grid || 24ull + a.wfirst[k] > a.cap) {
        a.out_total[0] = 0;
        a.out_total[1] = 24;
      }
    }
  }
  if (a.cap < 24) return;  // (uniform) no record fits
  const GQueue q = g_queue(a, grid);
  const uint64_t beg = (uint64_t)g * q.span;
  const uint64_t end = beg + q.span < q.m ? beg + q.span : q.m;
  if (beg >= end) return;  // (uniform)
  uint64_t B = 0, R = 0;   // the output offset and the number of the range's first record
  for (uint32_t k = t; k < g; k += kGTile) {
    B += a.wsum[k];
    R += a.wcnt[k];
  }
  B = 24 + block_sum(B, red, t);
  R = block_sum(R, red, t);
  uint32_t nwr = 0;      // records of this range written so far
  bool stopped = false;  // a record of this range did not fit: no later one does (the ends ascend)
  for (uint64_t tb = beg; tb < end && !stopped; tb += kGTile) {
    const uint64_t j = tb + t;
    PRec r;
    r.i = 0xFFFFFFFFu, r.len = r.incl = 0, r.src = a.frames;
    if (j < end) r = p_record(a, q, j);
    const bool valid = j < end && r.i < a.n;
    const uint32_t adv = valid ? 16 + r.incl : 0u;
    pre[t] = adv;
    tile_scan(pre, t);  // of the record sizes
    const uint64_t off = B + pre[t] - adv;  // the record's first byte
    const bool wr = valid && off + adv <= a.cap;
    len_s[t] = r.len;
    incl_s[t] = r.incl;
    idx_s[t] = r.i;
    src_s[t] = r.src;
    sc[t] = wr ? (1u << kPShift) | (1 + (r.incl + 15) / 16) : 0u;
    tile_scan(sc, t);  // of records written | chunks
    const uint32_t rank = sc[t] >> kPShift, wc = sc[kGTile - 1] >> kPShift;
    cpre[t] = sc[t] & kPMask;
    if (wr) {  // the written records are a prefix of the records: the rank is the record number
      const uint64_t rr = R + nwr + rank - 1;
      if (a.out_offsets) a.out_offsets[rr] = (uint32_t)(off + 16);
      if (a.out_lens) a.out_lens[rr] = (uint16_t)r.incl;
      if (rank == wc) last_end = (uint32_t)(off + adv);
    }
    stopped = __syncthreads_or(valid && !wr) != 0;
    // wave w copies the w-th quarter of the tile's chunks, lane l the chunks l, l + 64, ... of it,
    // four in flight before any store (gather_copy's deal)
    const uint32_t chunks = cpre[kGTile - 1];
    const uint32_t wv = t >> 6, ln = t & 63, qc = (chunks + 3) / 4;
    const uint32_t kb = min(wv * qc, chunks), ke = min(kb + qc, chunks);
    uint32_t p = 0;
    if (kb + ln < ke) {
      uint32_t lo = 0, hi = kGTile - 1;  // (cpre[kGTile - 1] > k for every k < chunks)
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cpre[mid] <= kb + ln) lo = mid + 1;
        else hi = mid;
      }
      p = lo;
    }
    for (uint32_t k0 = kb + ln; k0 < ke; k0 += 4 * 64) {
      u32x4 v[4];
      uint8_t* dst[4];
      uint32_t rem[4];  // 0: nothing, 16: the whole chunk, else that many bytes
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t k = k0 + 64 * u;
        rem[u] = 0;
        dst[u] = a.out;
        v[u] = u32x4{0u, 0u, 0u, 0u};
        if (k >= ke) continue;
        while (cpre[p] <= k) p++;
        const uint32_t c = k - (p ? cpre[p - 1] : 0u);
        const uint32_t lp = len_s[p], ip = incl_s[p];
        const uint8_t* sp = src_s[p];
        dst[u] = a.out + (B + pre[p] - (16 + ip) + 16ull * c);
        if (c == 0) {  // the record header
          rem[u] = 16;
          if ((a.flags & kPcapSrcRecords) && (uintptr_t)sp - (uintptr_t)a.frames >= 16) {
            const u32x4_any x = *(g_u4_any*)((uintptr_t)sp - 16);  // the source's own, as it lies
            const uint32_t cut = swap ? __builtin_bswap32(ip) : ip;
            v[u] = u32x4{x.x, x.y, ip < lp ? cut : x.z, x.w};
          } else {
            const uint32_t i = idx_s[p];
            const uint32_t s0 = a.ts ? a.ts[2ull * i] : i, s1 = a.ts ? a.ts[2ull * i + 1] : 0u;
            v[u] = swap ? u32x4{__builtin_bswap32(s0), __builtin_bswap32(s1),
                                __builtin_bswap32(ip), __builtin_bswap32(lp)}
                        : u32x4{s0, s1, ip, lp};
          }
          continue;
        }
        const uint32_t left = ip - 16 * (c - 1);
        if (left >= 16) {  // inside the packet: one load, as it lies
          const u32x4_any x = *(g_u4_any*)((uintptr_t)sp + 16ull * (c - 1));
          v[u] = u32x4{x.x, x.y, x.z, x.w};
          rem[u] = 16;
        } else {  // the last, partial chunk: the next record's header starts right behind it
          v[u] = tail_chunk(sp, ip, c - 1);
          rem[u] = left;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (rem[u] == 16) *(u32x4_any*)dst[u] = v[u];
        else if (rem[u]) store_bytes(dst[u], v[u], rem[u]);
      }
    }
    nwr += wc;
    B += pre[kGTile - 1];
    __syncthreads();  // (the next tile rewrites the LDS arrays)
  }
  if (t == 0 && nwr) {
    // this range's last written record is the last one of all iff the next record -- in this
    // range, else the first one of the next range that has any -- does not fit or does not exist
    bool last = stopped;
    if (!last) {  // (every record of the range was written: B is where the next one starts)
      uint32_t k = g + 1;
      while (k < grid && a.wcnt[k] == 0) k++;
      last = k == grid || B + a.wfirst[k] > a.cap;
    }
    if (last) {
      a.out_total[0] = (uint32_t)(R + nwr);
      a.out_total[1] = last_end;
    }
  }
}

// ============================================================================================
// Scatter: the gather reversed. Queue position j's destination (packet
// index[start + j] of the original batch) and its source (src_offsets[j] of the dense buffer) are
// both given, so there is no prefix across workgroups and one launch does it: the m positions are
// split into contiguous per-workgroup ranges of whole kGTile tiles as the gather's are; a thread
// per position merges the entry's results and works out its packet's copy, then the tile's chunks
// are dealt to the lanes as gather_copy deals its. The chunks are cut on the DESTINATION's
// 16-byte grid: chunk c of a packet at address D is the part of the aligned block (D & ~15) +
// 16 c that holds its bytes, so an inside chunk is one unaligned 16-byte load and one aligned
// 16-byte store, and only a packet's first and last chunk are partial. Other lanes (and other
// workgroups) write the bytes next to a partial chunk at the same time, so it is stored with
// naturally aligned 1/2/4/8-byte stores of exactly its bytes, never by a read-modify-write.
// ============================================================================================
typedef __attribute__((address_space(1))) u32x4 gs_u4;
typedef __attribute__((address_space(1))) uint64_t gs_u64;
typedef __attribute__((address_space(1))) uint32_t gs_u32;
typedef __attribute__((address_space(1))) uint16_t gs_u16;
typedef __attribute__((address_space(1))) uint8_t gs_u8;

// The first cnt (1..15) bytes of v to the address p, no byte more, p + cnt inside p's aligned
// 16-byte block: 1, 2, 4, 8 bytes while p's alignment asks for them and they fit, then 8, 4, 2, 1
// of what is left -- every store naturally aligned.
__device__ __forceinline__ void store_span(uintptr_t p, u32x4 v, uint32_t cnt) {
  uint64_t lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
  uint64_t hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
  if ((p & 1) && cnt >= 1) {
    *(gs_u8*)p = (uint8_t)lo;
    lo = (lo >> 8) | (hi << 56);
    hi >>= 8;
    p += 1, cnt -= 1;
  }
  if ((p & 2) && cnt >= 2) {
    *(gs_u16*)p = (uint16_t)lo;
    lo = (lo >> 16) | (hi << 48);
    hi >>= 16;
    p += 2, cnt -= 2;
  }
  if ((p & 4) && cnt >= 4) {
    *(gs_u32*)p = (uint32_t)lo;
    lo = (lo >> 32) | (hi << 32);
    hi >>= 32;
    p += 4, cnt -= 4;
  }
  if ((p & 8) && cnt >= 8) {
    *(gs_u64*)p = lo;
    lo = hi;
    p += 8, cnt -= 8;
  }
  // (a step skipped for room leaves p aligned to its size and fewer bytes than it: the stores
  // below, of cnt's bits from the highest down, are aligned too; else p is 16-byte aligned)
  if (cnt & 8) {
    *(gs_u64*)p = lo;
    lo = hi;
    p += 8;
  }
  if (cnt & 4) {
    *(gs_u32*)p = (uint32_t)lo;
    lo >>= 32;
    p += 4;
  }
  if (cnt & 2) {
    *(gs_u16*)p = (uint16_t)lo;
    lo >>= 16;
    p += 2;
  }
  if (cnt & 1) *(gs_u8*)p = (uint8_t)lo;
}

struct SQueue {
  uint32_t start, m;  // the positions scattered are index[start .. start + m)
  uint64_t span;      // queue positions per workgroup
};
__device__ __forceinline__ SQueue s_queue(const ScatterArgs& a, uint32_t grid) {
  uint64_t start = 0;
  for (uint32_t c = 0; c < a.queue; c++) start += a.count[c];
  uint64_t m = a.count[a.queue];
  // (counts that do not belong to this batch: stay inside index[0, n))
  if (start > a.n) start = a.n;
  if (m > a.n - start) m = a.n - start;
  if (m > a.cap) m = a.cap;
  if (a.total && m > a.total[0]) m = a.total[0];
  SQueue q;
  q.start = (uint32_t)start;
  q.m = (uint32_t)m;
  const uint64_t per = (m + grid - 1) / grid;
  q.span = (per + kGTile - 1) / kGTile * kGTile;
  return q;
}

__global__ __launch_bounds__(kGTile) void scatter_copy(ScatterArgs a) {
  __shared__ uint32_t cpre[kGTile], len_s[kGTile];
  __shared__ const uint8_t* src_s[kGTile];
  __shared__ uintptr_t dst_s[kGTile];
  const uint32_t t = threadIdx.x, g = blockIdx.x;
  const SQueue q = s_queue(a, gridDim.x);
  const uint64_t beg = (uint64_t)g * q.span;
  const uint64_t end = beg + q.span < q.m ? beg + q.span : q.m;
  for (uint64_t tb = beg; tb < end; tb += kGTile) {  // (uniform)
    const uint64_t j = tb + t;
    uint32_t L = 0;  // bytes of this position's packet to copy
    const uint8_t* S = a.src_frames;
    uintptr_t D = (uintptr_t)a.frames;
    if (j < end) {
      const uint64_t d = a.index[q.start + j];
      bool ok = d < a.n;
      if (ok && a.frames) {
        const uint64_t so = a.src_offsets[j];
        const uint32_t sl = a.src_lens[j];
        ok = so + sl <= a.src_bytes;
        if (ok) {
          const uint64_t dl = a.lens ? (uint64_t)a.lens[d] : a.stride;
          L = dl < sl ? (uint32_t)dl : sl;
          S = a.src_frames + so;
          D = (uintptr_t)a.frames + (a.offsets ? (uint64_t)a.offsets[d] : d * a.stride);
        }
      }
      if (ok) {  // a wrong index, a source span past the dense buffer: no results either
        if (a.verdict) a.verdict[d] = a.src_verdict[j];
        if (a.status) a.status[d] = a.src_status[j];
        if (a.r0) a.r0[d] = a.src_r0[j];
      }
    }
    if (!a.frames) continue;  // (uniform) results only
    len_s[t] = L;
    src_s[t] = S;
    dst_s[t] = D;
    // the aligned 16-byte blocks that hold a byte of [D, D + L)
    cpre[t] = L ? (uint32_t)(((D + L + 15) >> 4) - (D >> 4)) : 0u;
    __syncthreads();
    for (uint32_t d = 1; d < kGTile; d <<= 1) {  // inclusive scan of the chunk counts
      const uint32_t v = t >= d ? cpre[t - d] : 0u;
      __syncthreads();
      cpre[t] += v;
      __syncthreads();
    }
    // wave w copies the w-th quarter of the tile's chunks, lane l the chunks l, l + 64, ... of it,
    // four in flight before any store (gather_copy's deal)
    const uint32_t chunks = cpre[kGTile - 1];
    const uint32_t wv = t >> 6, ln = t & 63, qc = (chunks + 3) / 4;
    const uint32_t kb = min(wv * qc, chunks), ke = min(kb + qc, chunks);
    uint32_t p = 0;
    if (kb + ln < ke) {
      uint32_t lo = 0, hi = kGTile - 1;  // (cpre[kGTile - 1] > k for every k < chunks)
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cpre[mid] <= kb + ln) lo = mid + 1;
        else hi = mid;
      }
      p = lo;
    }
    for (uint32_t k0 = kb + ln; k0 < ke; k0 += 4 * 64) {
      u32x4 v[4];
      uintptr_t at[4];
      uint32_t cnt[4];  // 0: nothing, 16: the whole aligned block, else that many bytes at at[u]
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t k = k0 + 64 * u;
        cnt[u] = 0;
        at[u] = 0;
        v[u] = u32x4{0u, 0u, 0u, 0u};
        if (k >= ke) continue;
        while (cpre[p] <= k) p++;
        const uint32_t c = k - (p ? cpre[p - 1] : 0u);
        const uint32_t lp = len_s[p];
        const uint8_t* sp = src_s[p];
        const uintptr_t dp = dst_s[p];
        const uintptr_t blk = (dp & ~(uintptr_t)15) + 16ull * c;
        const uintptr_t lo = blk > dp ? blk : dp;
        const uintptr_t hi = blk + 16 < dp + lp ? blk + 16 : dp + lp;
        const uint32_t off = (uint32_t)(lo - dp);  // the chunk's first byte inside the packet
        at[u] = lo;
        cnt[u] = (uint32_t)(hi - lo);
        if (cnt[u] == 16) {  // inside the packet: one load, as it lies
          const u32x4_any x = *(g_u4_any*)((uintptr_t)sp + off);
          v[u] = u32x4{x.x, x.y, x.z, x.w};
        } else {
          v[u] = span_load(sp, lp, off, cnt[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (cnt[u] == 16) *(gs_u4*)at[u] = v[u];
        else if (cnt[u]) store_span(at[u], v[u], cnt[u]);
      }
    }
    __syncthreads();  // (the next tile rewrites the LDS arrays)
  }
}

}  // namespace

hipError_t launch_queues(const uint8_t* verdict, uint64_t n, uint32_t* index, uint32_t* count,
                         uint8_t* ws, hipStream_t stream) {
  const uint64_t g = (n + kQRange - 1) / kQRange;
  const int grid = (int)(g < 1 ? 1 : g > (uint64_t)kQMaxWgs ? (uint64_t)kQMaxWgs : g);
  uint32_t* wgc = (uint32_t*)ws;
  uint32_t* wvc = (uint32_t*)(ws + kQWsWaveOff);
  hipLaunchKernelGGL(queues_count, dim3(grid), dim3(kQBlock), 0, stream, verdict, n, wgc, wvc);
  hipLaunchKernelGGL(queues_scatter, dim3(grid), dim3(kQBlock), 0, stream, verdict, n, wgc, wvc,
                     index, count);
  return hipGetLastError();
}

hipError_t launch_gather(const GatherArgs& a, hipStream_t stream) {
  const uint64_t g = (a.n + kGTile - 1) / kGTile;
  const int grid = (int)(g < 1 ? 1 : g > (uint64_t)kGMaxWgs ? (uint64_t)kGMaxWgs : g);
  hipLaunchKernelGGL(gather_sums, dim3(grid), dim3(kGTile), 0, stream, a);
  hipLaunchKernelGGL(gather_copy, dim3(grid), dim3(kGTile), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_pcap_gather(const PcapArgs& a, hipStream_t stream) {
  const uint64_t g = (a.n + kGTile - 1) / kGTile;
  const int grid = (int)(g < 1 ? 1 : g > (uint64_t)kGMaxWgs ? (uint64_t)kGMaxWgs : g);
  hipLaunchKernelGGL(pcap_sums, dim3(grid), dim3(kGTile), 0, stream, a);
  hipLaunchKernelGGL(pcap_copy, dim3(grid), dim3(kGTile), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_scatter(const ScatterArgs& a, hipStream_t stream) {
  const uint64_t g = ((uint64_t)a.cap + kGTile - 1) / kGTile;
  const int grid = (int)(g < 1 ? 1 : g > (uint64_t)kGMaxWgs ? (uint64_t)kGMaxWgs : g);
  hipLaunchKernelGGL(scatter_copy, dim3(grid), dim3(kGTile), 0, stream, a);
  return hipGetLastError();
}

}  // namespace ebpfemu
