// csum.hip — checksum offload: what a NIC's RX descriptor says about the IPv4
// header checksum and the TCP / UDP checksum of every packet of a batch (ebpf_csum_verify), and the
// TX side that writes them (ebpf_csum_fill). New: no reference counterpart (the reference runs one
// packet and prints r0); the parse and the sums follow include/ebpf_emu.h.
//
// A wave takes 64 packets. One lane per packet parses the headers (steer.hip's rss_hash idiom) and
// sums what is short: the IPv4 header and the pseudo-header. The L4 spans of the 64 packets, 8 bytes
// to 64 KiB long, are cut into aligned 16-byte blocks and laid end to end; the wave's lanes walk
// that list 64 blocks a step (lane j: blocks j, j + 64, ...), each finding its block's owner in the
// prefix sums, loading one dwordx4, masking the bytes outside the span and adding the block's word
// sum into the owner's LDS slot. So the loads are 16 bytes a lane, neighbouring lanes read
// neighbouring blocks, and a 1500-byte packet next to a 64-byte one costs no divergence.
//
// The discipline of queues.hip and steer.hip: no workgroup waits on another, no device atomics, no
// grid barrier, no cooperative launch; a capped grid walks a larger batch in passes. The only LDS
// atomics add up sums whose order does not matter.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ebpf_emu.h"
#include "launch.h"

namespace ebpfemu {
namespace {

typedef __attribute__((address_space(1))) const uint32_t g_u32;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const u32x4 g_u32x4;

__device__ __forceinline__ uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// (steer.hip's packet reads, copied) The aligned dword at a, read only where it holds a byte of the
// packet [.., end) (every a here is past the packet's first byte).
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

// The sums are taken over the 16-bit words as a little-endian load gives them and byte-swapped
// once they are folded (RFC 1071 §2(B): the one's complement sum is byte-order independent).
__device__ __forceinline__ uint32_t halves(uint32_t w) { return (w & 0xFFFFu) + (w >> 16); }
__device__ __forceinline__ uint32_t fold(uint32_t t) {  // t <= 2^32 - 1: two rounds reach 16 bits
  t = (t & 0xFFFFu) + (t >> 16);
  t = (t & 0xFFFFu) + (t >> 16);
  return (t & 0xFFFFu) + (t >> 16);
}
__device__ __forceinline__ uint32_t swap16(uint32_t x) { return ((x & 0xFFu) << 8) | (x >> 8); }

// 4 byte-enable bits -> a mask of 4 bytes (bit k lands on bit 8k: 0x00204081 = 1 + 2^7 + 2^14 + 2^21).
__device__ __forceinline__ uint32_t byte_mask(uint32_t nib) {
  return (((nib & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int s = 32; s; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s, 64);
  return v;
}

constexpr uint32_t kNoField = 0xFFFFu;  // meta's field offset: nothing to mask (verify)

template <bool FILL>
__global__ __launch_bounds__(kCsBlock) void csum_kernel(CsumArgs a) {
  // per wave, per packet: the span's blocks (inclusive / exclusive prefix), its first byte, its
  // length | the field's offset inside it << 16, and the sum
  __shared__ uint32_t incl[kCsWaves][64], excl[kCsWaves][64], meta[kCsWaves][64], acc[kCsWaves][64];
  __shared__ uint64_t first[kCsWaves][64];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  // (the bound is the workgroup's: every wave of it makes every pass and meets every barrier)
  for (uint64_t i0 = (uint64_t)blockIdx.x * kCsBlock; i0 < a.n; i0 += (uint64_t)gridDim.x * kCsBlock) {
    const uint64_t i = i0 + t;
    const bool in = i < a.n;
    bool on = in;
    if (in && a.verdict) {
      const uint32_t v = a.verdict[i];
      const uint32_t q = v < 5 ? v : v == 0xFFu ? 6u : 5u;
      on = (a.queue_mask >> q) & 1u;
    }
    const uintptr_t s0 = (uintptr_t)a.frames + (in ? (a.offsets ? (uint64_t)a.offsets[i] : i * a.stride) : 0);
    const uint32_t len = !in ? 0u : a.lens ? (uint32_t)a.lens[i] : (uint32_t)a.stride;
    const uintptr_t end = s0 + len;
    // L2: the ethertypes at 12, 16 and 20; each is looked at only once len covers it
    uint32_t e[3];
    pkt_words<3>(s0 + 12, end, on, e);
    uint32_t o = 14, et = be16(e[0]);
    bool ok = on && len >= 14;
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
    // the IP header's first 20 bytes, and the next 20 of an IPv6 one
    uint32_t w[5], y[5] = {0u, 0u, 0u, 0u, 0u};
    pkt_words<5>(s0 + o, end, v4 || v6, w);
    if (ballot(v6) != 0) pkt_words<5>(s0 + o + 20, end, v6, y);  // (uniform)
    const uint32_t ver = (w[0] >> 4) & 15u, ihl = w[0] & 15u, H = 4 * ihl;
    v4 = v4 && ver == 4 && ihl >= 5 && len >= o + H;
    v6 = v6 && ver == 6;
    uint32_t st = 0;

    // L3: the IPv4 header, by its own lane (20 bytes are in registers; options are rare)
    if (v4 && (a.what & EBPF_CSUM_IPV4_HDR)) {
      uint32_t s = halves(w[0]) + halves(w[1]) + (FILL ? w[2] & 0xFFFFu : halves(w[2])) + halves(w[3]) +
                   halves(w[4]);
      for (uint32_t k = 5; k < ihl; k++) {
        uint32_t x[1];
        pkt_words<1>(s0 + o + 4 * k, end, true, x);
        s += halves(x[0]);
      }
      s = fold(s);
      if (FILL) {  // ~sum, big-endian: the little-endian sum's low byte is the field's first
        uint8_t* f = (uint8_t*)(s0 + o + 10);
        f[0] = (uint8_t)~s;
        f[1] = (uint8_t)(~s >> 8);
        st |= EBPF_CSUM_L3_GOOD;
      } else {
        st |= s == 0xFFFFu ? EBPF_CSUM_L3_GOOD : EBPF_CSUM_L3_BAD;
      }
    }

    // L4: the span [p, p + L), the pseudo-header's addresses (little-endian halves) and protocol
    const uint32_t tot = be16(w[0] >> 16);                        // IPv4: be16 at o + 2
    const bool frag = (be16(w[1] >> 16) & 0x3FFFu) != 0;          //       be16 at o + 6
    const uint32_t proto = v4 ? (w[2] >> 8) & 0xFFu : (w[1] >> 16) & 0xFFu;  // o + 9, o + 6
    const uint32_t p = v4 ? o + H : o + 40;
    const uint32_t L = v4 ? tot - H : be16(w[1]);                 // IPv6: be16 at o + 4
    const bool whole = v4 ? tot >= H && o + tot <= len && !frag : v6 && p + L <= len;
    uint32_t ps = halves(w[3]) + halves(w[4]);
    if (v6) ps += halves(w[2]) + halves(y[0]) + halves(y[1]) + halves(y[2]) + halves(y[3]) + halves(y[4]);
    const bool tcp = whole && proto == 6 && (a.what & EBPF_CSUM_TCP) && L >= 20;
    bool udp = whole && proto == 17 && (a.what & EBPF_CSUM_UDP) && L >= 8;
    uint32_t u[1] = {0u};  // UDP's length and checksum fields, p + 4 .. p + 8
    if (ballot(udp) != 0) pkt_words<1>(s0 + p + 4, end, udp, u);  // (uniform)
    udp = udp && be16(u[0]) == L;
    const bool none = !FILL && udp && v4 && (u[0] >> 16) == 0;  // UDP over IPv4, none sent
    const bool sum = (tcp || udp) && !none;
    const uint32_t foff = tcp ? 16u : 6u;
    const uintptr_t pb = s0 + p, pe = pb + L;
    const uint32_t cnt = sum ? (uint32_t)(((pe + 15) >> 4) - (pb >> 4)) : 0u;  // L >= 8: pe > pb
    uint32_t run = cnt;  // inclusive prefix over the wave
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)run, s, 64);
      run += lane >= (uint32_t)s ? up : 0u;
    }
    incl[wv][lane] = run;
    excl[wv][lane] = run - cnt;
    meta[wv][lane] = L | ((FILL ? foff : kNoField) << 16);
    first[wv][lane] = pb;
    acc[wv][lane] = 0;
    __syncthreads();

    // the wave's block list, 64 blocks a step
    const uint32_t total = __builtin_amdgcn_readfirstlane(incl[wv][63]);
    for (uint32_t b0 = 0; b0 < total; b0 += 64) {
      const uint32_t b = b0 + lane;
      const bool act = b < total;
      uint32_t k = 0;  // the owner: the first packet whose inclusive prefix passes b
#pragma unroll
      for (uint32_t s = 32; s; s >>= 1) k += incl[wv][k + s - 1] <= b ? s : 0u;
      uint32_t v = 0;
      if (act) {
        const uint64_t kb = first[wv][k];
        const uint32_t m = meta[wv][k];
        const uint64_t ke = kb + (m & 0xFFFFu);
        const uint64_t A = (kb & ~15ull) + 16ull * (b - excl[wv][k]);
        const u32x4 d = *(g_u32x4*)A;
        const uint32_t lo = kb > A ? (uint32_t)(kb - A) : 0u;
        const uint32_t hi = ke < A + 16 ? (uint32_t)(ke - A) : 16u;
        uint32_t bm = ((1u << hi) - 1u) & ~((1u << lo) - 1u);  // the bytes of the span
        if (FILL) {  // the field's two bytes count as 0
          const int64_t df = (int64_t)(kb + (m >> 16)) - (int64_t)A;
          if (df >= -1 && df < 16) bm &= ~(df < 0 ? 1u : 3u << df);
        }
        v = halves(d.x & byte_mask(bm)) + halves(d.y & byte_mask(bm >> 4)) +
            halves(d.z & byte_mask(bm >> 8)) + halves(d.w & byte_mask(bm >> 12));
      }
      // one packet's blocks all along the step (inside a long span): one add for the wave
      const uint32_t kf = __builtin_amdgcn_readfirstlane(k);  // (lane 0 is active: b0 < total)
      if (ballot(act && k != kf) == 0) {                      // (uniform)
        v = wave_sum(v);
        if (lane == 0) atomicAdd(&acc[wv][kf], v);
      } else if (act) {
        atomicAdd(&acc[wv][k], v);  // (a sum: the order does not matter)
      }
    }
    __syncthreads();

    if (sum) {
      // the blocks were summed as they lie: a span at an odd address has its bytes in the other
      // halves of the 16-bit words, which is the byte swap the big-endian sum wants anyway
      const uint32_t x = fold(acc[wv][lane]);
      const uint32_t body = (pb & 1) ? x : swap16(x);
      const uint32_t c = fold(swap16(fold(ps)) + proto + L + body);
      if (FILL) {
        uint32_t val = ~c & 0xFFFFu;
        if (udp && val == 0) val = 0xFFFFu;
        uint8_t* f = (uint8_t*)(pb + foff);
        f[0] = (uint8_t)(val >> 8);
        f[1] = (uint8_t)val;
        st |= EBPF_CSUM_L4_GOOD;
      } else {
        st |= c == 0xFFFFu ? EBPF_CSUM_L4_GOOD : EBPF_CSUM_L4_BAD;
      }
    } else if (none) {
      st |= EBPF_CSUM_L4_NONE;
    }
    if (in && a.status) a.status[i] = (uint8_t)st;
  }
}

}  // namespace

hipError_t launch_csum(const CsumArgs& c, bool fill, hipStream_t stream) {
  const uint64_t g = (c.n + kCsBlock - 1) / kCsBlock;
  const int grid = (int)(g < 1 ? 1 : g > (uint64_t)kCsMaxWgs ? (uint64_t)kCsMaxWgs : g);
  if (fill)
    hipLaunchKernelGGL(csum_kernel<true>, dim3(grid), dim3(kCsBlock), 0, stream, c);
  else
    hipLaunchKernelGGL(csum_kernel<false>, dim3(grid), dim3(kCsBlock), 0, stream, c);
  return hipGetLastError();
}

}  // namespace ebpfemu
