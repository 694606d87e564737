// steer.hip — RSS flow steering: the Toeplitz hash a NIC puts in the RX
// descriptor (ebpf_rss_hash) and the stable partition of the packet numbers into up to 64 receive
// queues by the indirection table (ebpf_steer). New: no reference counterpart (the reference runs
// one packet and prints r0); the hash and the parse follow include/ebpf_emu.h.
//
// The partition keeps the discipline of queues.hip: count -> bases -> write over contiguous
// per-workgroup ranges, in separate launches: the launch boundary is the only ordering between
// workgroups. No workgroup ever waits on another one's progress (no look-back, no flag, no grid
// barrier, no cooperative launch), so a grid larger than the resident set cannot hang. No device
// atomics; the only LDS atomics add up sums whose order does not matter.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "launch.h"

namespace ebpfemu {
namespace {

typedef __attribute__((address_space(1))) const uint32_t g_u32;

__device__ __forceinline__ uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// ============================================================================================
// The hash. One lane per packet, packet i = (pass * grid + workgroup) * kRssBlock + thread. A lane
// parses its packet's headers from aligned dwords, funnel-shifted (queues.hip q_load4's idiom), each
// read only where it holds a byte of the packet: at most 4 dwords of L2, 6 of the IP header, 7 more
// of an IPv6 header, 2 of an IPv4 packet's ports. The input words are then hashed bit by bit against
// the key windows, which are launch arguments read by constant index and so sit in scalar
// registers: per input bit one v_bfe_i32 (the bit, sign-extended), one v_and with the window, one
// v_xor. No LDS. The input words 3..8 exist for IPv6 only and are skipped by a wave without one.
// ============================================================================================

// The aligned dword at a, read only where it holds a byte of the packet [.., end) (every a here is
// past the packet's first byte).
__device__ __forceinline__ uint32_t pkt_dword(uintptr_t a, uintptr_t end, bool on) {
  return (on && a < end) ? *(g_u32*)a : 0u;
}

// The K dwords of packet bytes at p, p + 4, ... (any alignment of p), byte 0 in the low bits. Bytes
// at or past end are unspecified.
template <int K>
__device__ __forceinline__ void pkt_words(uintptr_t p, uintptr_t end, bool on, uint32_t (&w)[K]) {
  const uintptr_t a = p & ~(uintptr_t)3;
  const uint32_t sh = (uint32_t)(p & 3);
  uint32_t d[K + 1];
#pragma unroll
  for (int k = 0; k <= K; k++) d[k] = pkt_dword(a + 4 * k, end, on);
#pragma unroll
  for (int k = 0; k < K; k++) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
}

// The big-endian 16-bit field in a word's first two bytes.
__device__ __forceinline__ uint32_t be16(uint32_t w) { return ((w & 0xFFu) << 8) | ((w >> 8) & 0xFFu); }
__device__ __forceinline__ bool is_vlan(uint32_t et) { return et == 0x8100u || et == 0x88A8u; }

typedef __attribute__((address_space(4))) const uint32_t k_u32;

// The key windows as they lie in the kernel's argument block (RssArgs is its only argument). The
// pointer is made opaque once per packet, so the window loads stay inside the packet loop: hoisted
// out of it, 288 live scalar values would spill.
__device__ __forceinline__ k_u32* rss_windows() {
  k_u32* p = (k_u32*)((__attribute__((address_space(4))) const char*)__builtin_amdgcn_kernarg_segment_ptr() +
                      offsetof(RssArgs, win));
  asm volatile("" : "+s"(p));
  return p;
}

template <int K0, int K1>
__device__ __forceinline__ uint32_t toeplitz(k_u32* win, const uint32_t (&x)[9], uint32_t h) {
#pragma unroll
  for (int k = K0; k < K1; k++) {
#pragma unroll
    for (int b = 0; b < 32; b++) h ^= (uint32_t)((int32_t)(x[k] << b) >> 31) & win[32 * k + b];
  }
  return h;
}

__global__ __launch_bounds__(kRssBlock) void rss_hash(RssArgs a) {
  for (uint64_t i = (uint64_t)blockIdx.x * kRssBlock + threadIdx.x; i < a.n;
       i += (uint64_t)gridDim.x * kRssBlock) {
    const uintptr_t s0 = (uintptr_t)a.frames + (a.offsets ? (uint64_t)a.offsets[i] : i * a.stride);
    const uint32_t len = a.lens ? (uint32_t)a.lens[i] : (uint32_t)a.stride;
    const uintptr_t end = s0 + len;
    // L2: the ethertypes at 12, 16 and 20; each is looked at only once len covers it
    uint32_t e[3];
    pkt_words<3>(s0 + 12, end, true, e);
    uint32_t o = 14, et = be16(e[0]);
    bool ok = len >= 14;
    const bool t1 = ok && is_vlan(et);
    o = t1 ? 18u : o;
    ok = t1 ? len >= 18 : ok;
    et = t1 ? be16(e[1]) : et;
    const bool t2 = t1 && ok && is_vlan(et);
    o = t2 ? 22u : o;
    ok = t2 ? len >= 22 : ok;
    et = t2 ? be16(e[2]) : et;
    ok = ok && !(t2 && is_vlan(et));  // a third tag
    bool v4 = ok && et == 0x0800u && len >= o + 20;
    bool v6 = ok && et == 0x86DDu && len >= o + 40;
    // the IP header's first 20 bytes, and the next 24 of an IPv6 one
    uint32_t w[5], y[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    pkt_words<5>(s0 + o, end, v4 || v6, w);
    const bool any6 = ballot(v6) != 0;  // (uniform)
    if (any6) pkt_words<6>(s0 + o + 20, end, v6, y);
    const uint32_t ver = (w[0] >> 4) & 15u, ihl = w[0] & 15u;
    v4 = v4 && ver == 4 && ihl >= 5;
    v6 = v6 && ver == 6;
    const uint32_t proto = v4 ? (w[2] >> 8) & 0xFFu : (w[1] >> 16) & 0xFFu;  // o + 9, o + 6
    const bool frag = v4 && (be16(w[1] >> 16) & 0x3FFFu) != 0;               // be16 at o + 6
    const uint32_t tcp = v4 ? 2u : 16u, udp = v4 ? 4u : 32u, ip = v4 ? 1u : 8u;
    const uint32_t l4 = proto == 6 ? tcp : proto == 17 ? udp : 0u;
    const uint32_t pat = v4 ? o + 4 * ihl : o + 40;  // the ports
    const bool ports = (v4 || v6) && !frag && (l4 & a.types) != 0 && len >= pat + 4;
    const uint32_t ty = ports ? l4 : (v4 || v6) ? (ip & a.types) : 0u;
    uint32_t pw[1] = {0u};
    if (ballot(ports && v4) != 0) pkt_words<1>(s0 + pat, end, ports && v4, pw);  // (uniform)
    // the input, big-endian words: bit 31 of x[0] is input bit 0
    uint32_t x[9];
    const bool h4 = v4 && ty != 0, h6 = v6 && ty != 0;
    x[0] = h4 ? w[3] : h6 ? w[2] : 0u;
    x[1] = h4 ? w[4] : h6 ? w[3] : 0u;
    x[2] = h4 ? (ports ? pw[0] : 0u) : h6 ? w[4] : 0u;
#pragma unroll
    for (int k = 3; k < 8; k++) x[k] = h6 ? y[k - 3] : 0u;
    x[8] = (h6 && ports) ? y[5] : 0u;
#pragma unroll
    for (int k = 0; k < 9; k++) x[k] = __builtin_bswap32(x[k]);
    k_u32* win = rss_windows();
    uint32_t h = toeplitz<0, 3>(win, x, 0u);
    if (any6) h = toeplitz<3, 9>(win, x, h);
    a.hash[i] = h;
    if (a.type) a.type[i] = (uint8_t)ty;
  }
}

// ============================================================================================
// The partition. Workgroup g owns the keys [g * S, (g + 1) * S), S a whole number of kSRange (one
// while the grid is not capped); wave w of it the w-th quarter, walked 64 keys a step with lane =
// key, so the packet order is (workgroup, wave, step, lane). A key's class is its queue:
// reta[key & mask], the table in LDS.
//   steer_count: per-wave class counts (LDS atomics: a histogram) -> wvc[g][w][64], their
//     workgroup sums -> wgc[g][64].
//   steer_bases: ONE workgroup turns wgc into exclusive bases in place -- base[g][c] = keys of
//     lower classes + keys of class c in earlier workgroups -- and writes bounds. With 64 classes
//     this is what every write workgroup would otherwise redo for itself.
//   steer_write: every wave writes its keys' numbers from base(class) = base[g][c] + earlier waves'
//     of the class, kept per wave in LDS. One ballot per class does not scale to 64 classes: a
//     lane's rank inside its class is the number of lower lanes of the same class, from the mask
//     of lanes that agree with it on every class bit (one ballot per bit, `bits` of them).
// ============================================================================================
struct SSpan {
  uint64_t beg, end;
};
__device__ __forceinline__ SSpan s_wave_span(uint64_t n, uint32_t grid, uint32_t g, uint32_t w) {
  const uint64_t per = (n + grid - 1) / grid;
  const uint64_t S = (per + kSRange - 1) / kSRange * kSRange;
  const uint64_t q = S / kSWaves;  // a multiple of 64
  SSpan s;
  s.beg = (uint64_t)g * S + (uint64_t)w * q;
  s.end = s.beg + q;
  if (s.beg > n) s.beg = n;
  if (s.end > n) s.end = n;
  return s;
}

__global__ __launch_bounds__(kSBlock) void steer_count(SteerArgs a) {
  __shared__ uint32_t h[kSWaves][kSClasses];
  __shared__ uint8_t reta[kSReta];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6, g = blockIdx.x;
  if (t < (uint32_t)kSReta) reta[t] = a.reta[t];
  h[w][lane] = 0;
  __syncthreads();
  const SSpan sp = s_wave_span(a.n, gridDim.x, g, w);
  for (uint64_t e = sp.beg; e < sp.end; e += 64) {
    const uint64_t i = e + lane;
    if (i < sp.end) atomicAdd(&h[w][reta[a.key[i] & a.mask]], 1u);  // (sums: order does not matter)
  }
  __syncthreads();
  a.wvc[((uint64_t)g * kSWaves + w) * kSClasses + lane] = h[w][lane];
  if (t < (uint32_t)kSClasses) {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kSWaves; k++) sum += h[k][t];
    a.wgc[(uint64_t)g * kSClasses + t] = sum;
  }
}

// One workgroup of kSBasesBlock threads: thread (p, c) owns class c of the p-th part of the rows.
constexpr int kSBasesParts = 16;
constexpr int kSBasesBlock = kSBasesParts * kSClasses;
__global__ __launch_bounds__(kSBasesBlock) void steer_bases(SteerArgs a, uint32_t rows) {
  __shared__ uint32_t part[kSBasesParts][kSClasses], start[kSClasses], tot[kSClasses];
  const uint32_t t = threadIdx.x, c = t % kSClasses, p = t / kSClasses;
  const uint32_t per = (rows + kSBasesParts - 1) / kSBasesParts;
  const uint32_t r0 = min(p * per, rows), r1 = min(r0 + per, rows);
  uint32_t sum = 0;
  for (uint32_t r = r0; r < r1; r++) sum += a.wgc[(uint64_t)r * kSClasses + c];
  part[p][c] = sum;
  __syncthreads();
  if (t < (uint32_t)kSClasses) {
    uint32_t s = 0;
    for (int k = 0; k < kSBasesParts; k++) s += part[k][t];
    tot[t] = s;
  }
  __syncthreads();
  if (t < (uint32_t)kSClasses) {
    uint32_t s = 0;
    for (uint32_t k = 0; k < t; k++) s += tot[k];
    start[t] = s;
    if (t < a.nq) {
      a.bounds[2 * t] = s;
      a.bounds[2 * t + 1] = tot[t];
    }
  }
  __syncthreads();
  uint32_t run = start[c];
  for (uint32_t k = 0; k < p; k++) run += part[k][c];
  for (uint32_t r = r0; r < r1; r++) {
    const uint32_t v = a.wgc[(uint64_t)r * kSClasses + c];
    a.wgc[(uint64_t)r * kSClasses + c] = run;  // (read once, by this thread, before it is written)
    run += v;
  }
}

__global__ __launch_bounds__(kSBlock) void steer_write(SteerArgs a) {
  // (volatile: a class's base is read by every lane of the class and written back by its last
  // one, step after step -- kept in program order)
  __shared__ volatile uint32_t wb[kSWaves][kSClasses];
  __shared__ uint8_t reta[kSReta];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6, g = blockIdx.x;
  if (t < (uint32_t)kSReta) reta[t] = a.reta[t];
  {
    uint32_t b = a.wgc[(uint64_t)g * kSClasses + lane];  // class = lane
    for (uint32_t k = 0; k < w; k++) b += a.wvc[((uint64_t)g * kSWaves + k) * kSClasses + lane];
    wb[w][lane] = b;
  }
  __syncthreads();
  const SSpan sp = s_wave_span(a.n, gridDim.x, g, w);
  const uint64_t below = (1ull << lane) - 1;
  for (uint64_t e = sp.beg; e < sp.end; e += 64) {
    const uint64_t i = e + lane;
    const bool have = i < sp.end;
    const uint32_t c = have ? reta[a.key[i] & a.mask] : 0u;
    uint64_t m = ballot(have);  // -> the lanes of this lane's class
    for (uint32_t b = 0; b < a.bits; b++) {
      const bool bit = (c >> b) & 1;
      const uint64_t bal = ballot(bit);
      m &= bit ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(m & below), size = (uint32_t)__popcll(m);
    const uint32_t pos = wb[w][c] + rank;
    __builtin_amdgcn_wave_barrier();
    if (have && rank + 1 == size) wb[w][c] = pos + 1;
    __builtin_amdgcn_wave_barrier();
    // (keys that changed between the launches: stay inside index[0, n))
    if (have && pos < a.n) a.index[pos] = (uint32_t)i;
  }
}

}  // namespace

hipError_t launch_rss_hash(const RssArgs& r, hipStream_t stream) {
  const uint64_t g = (r.n + kRssBlock - 1) / kRssBlock;
  const int grid = (int)(g < 1 ? 1 : g > (uint64_t)kRssMaxWgs ? (uint64_t)kRssMaxWgs : g);
  hipLaunchKernelGGL(rss_hash, dim3(grid), dim3(kRssBlock), 0, stream, r);
  return hipGetLastError();
}

hipError_t launch_steer(const SteerArgs& s, hipStream_t stream) {
  const uint64_t g = (s.n + kSRange - 1) / kSRange;
  const int grid = (int)(g < 1 ? 1 : g > (uint64_t)kSMaxWgs ? (uint64_t)kSMaxWgs : g);
  hipLaunchKernelGGL(steer_count, dim3(grid), dim3(kSBlock), 0, stream, s);
  hipLaunchKernelGGL(steer_bases, dim3(1), dim3(kSBasesBlock), 0, stream, s, (uint32_t)grid);
  hipLaunchKernelGGL(steer_write, dim3(grid), dim3(kSBlock), 0, stream, s);
  return hipGetLastError();
}

}  // namespace ebpfemu
