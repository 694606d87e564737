// launch.h — host <-> device-launcher interface inside libebpfemu.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jit.h"
#include "uop.h"

namespace ebpfemu {

constexpr int kWave = 64;
constexpr int kBlock = 256;           // 4 waves per workgroup
constexpr int kWavesPerBlock = kBlock / kWave;
// the compiled fixed-slot kernel: one workgroup of 16 waves per CU, its tiles handed out to
// the waves by an LDS counter (interp.hip tile_body)
constexpr int kDbWaves = 16;
constexpr int kDbBlock = kDbWaves * kWave;
// ebpf_tile_jit_fixed_occ (issue-bound programs): one window buffer per wave, 3 workgroups of 8
// waves per CU (6 waves per SIMD, the limit of its ~103 SGPRs)
constexpr int kOccWaves = 8;
constexpr int kOccBlock = kOccWaves * kWave;
constexpr int kOccWgsPerCu = 3;
// its wide form (ebpf_tile_jit_fixed_occw): 2 workgroups of 12 waves per CU -- the same 6 waves per
// SIMD in fewer, larger workgroups -- for programs of at least kOccWideUops micro-ops (the rule
// chains: 53 -> 57 Gpkt/s at two streams for acl_rules, while the 5-tuple's line drops 106 -> 101
// on it: DESIGN 3.35). jit.cpp gives each program's code to the one of the two its length picks.
constexpr int kOccWideWaves = 12;
constexpr int kOccWideBlock = kOccWideWaves * kWave;
constexpr int kOccWideWgsPerCu = 2;
constexpr uint32_t kOccWideUops = 256;
constexpr int kWin = 64;              // packet bytes staged in LDS per lane (header window)
constexpr int kWinStride = kWin + 4;  // padded per-lane LDS stride: 17 dwords, conflict-free b32
constexpr int kMaxLdsUops = 4096;     // programs up to this many micro-ops are staged in LDS
constexpr int kCallDepth = 64;        // EBPF_MAX_CALL_DEPTH
constexpr int kCounterShards = 64;    // device-atomic counter shards (spread contention)
// workspace layout: [deopt count, done u32[2] @0 | (unused) | multi-GPU counter sums u64[8] @256 | xdp_md cursor u64 @320 |
// length-bin counts u32[16] @384 | bin cursors u32[16] @448, 512 B][shards u64[64][8]][tier-1
// wave slots, or the length-binned packet order u32[n]]; bin counts/cursors and shards are zero
// between batches
constexpr uint64_t kWsBinCountsOff = 384;
constexpr uint64_t kWsBinCursorOff = 448;
constexpr int kBinClasses = 16;  // packets are binned by ceil(len / 128), capped
constexpr int kBinMaxWgs = 1024;  // binning grid cap; per-workgroup class counts follow the order
constexpr uint64_t kWsDeoptOff = 0;  // u32 count, done: the deopt list (LaunchArgs::deopt); u32
                                     // at +8: how many packets the last deopt pass re-ran
constexpr uint64_t kWsXdpCursorOff = 320;  // u64: bytes staged by xdp_stage (reset per batch)
constexpr uint64_t kWsMultiOff = 256;  // u64[8]: ebpf_run_batch_multi's per-shard counter sums
constexpr uint64_t kWsShardsOff = 512;
constexpr uint64_t kWsSlotsOff = kWsShardsOff + kCounterShards * 8 * 8;

// Kernel kinds: the two memory tiers of interp_kernel, and dag_kernel (tier-0 programs whose
// jumps all go forward, run with max_steps >= n_uops so no step budget can bind).
enum KernelKind : int { kKindTier0 = 0, kKindTier1 = 1, kKindDag = 2, kKindLoop = 3 };
constexpr uint32_t kMaxDagUops = 256;

struct LaunchArgs {
  const Uop* prog;      // device micro-ops
  const DUop* dprog;    // device DAG micro-ops (kKindDag)
  const TUop* tprog;    // device tile micro-ops (kKindDag / kKindLoop, <= 62 micro-ops), else null
  const TUop* tprog_exact;  // kKindLoop: the one-micro-op-per-block table (exact step budget)
  uint32_t n_uops;
  uint32_t mem_size;
  const uint8_t* frames;
  const uint32_t* offsets;
  const uint16_t* lens;
  uint64_t stride;
  uint64_t n;
  uint64_t r10;
  uint64_t max_steps;
  uint8_t* verdict;
  uint64_t* r0;
  uint8_t* status;
  uint64_t* counters;   // optional caller counters [8] (added to)
  uint64_t* shards;     // workspace: [kCounterShards][8] partial counters (left zeroed)
  uint8_t* image_ws;    // tier 1: per-wave-slot images + call stacks
  uint64_t n_tiles;     // ceil(n / 64)
  const uint64_t* init_regs;  // optional [11] initial registers (else main.rs layout)
  uint8_t* mem_out;           // optional [n][mem_size] final images
  uint64_t* regs_out;         // optional [n][11] final registers
  uint32_t fold_kernel;       // 1: shards are folded by fold_counters after the launch, 0:
                              //    in-kernel (counted shard words, flush_counters)
  const uint32_t* perm;       // loop mode: packet index of tile slot i (length-binned), else null
  uint32_t* bin_counts;       // with perm: bin counts + cursors, zeroed again by the tile kernel
  uint64_t* trace;            // diagnostics (EBPFEMU_TRACE=1): per-wave s_memrealtime stamps of
                              // the compiled fixed-slot kernel, kTraceSlots per wave; else null
  const uint32_t* init_fp;    // tier-1 kernel: initial frame stack (Emu.fp, emu.rs:26), bottom first
  uint32_t init_fp_len;       //   its depth (<= kCallDepth)
  uint32_t* fp_out;           // tier-1 kernel: optional [n][kCallDepth] final frame stacks
  uint8_t* fp_len_out;        //   optional [n] their depths
  uint32_t xdp;               // 1: the xdp_md convention run in place (xdp.rs:16-20): image =
                              //   [u32 data = 8][u32 data_end = 8 + len][packet]; the window is
                              //   shifted by 8 bytes in LDS and the ctx synthesised per lane, BASE
                              //   = packet - 8 and LEN = 8 + len (no staging copy)
  // store-mode programs (jit.h StackPlan::any_dyn): the deopt list in the workspace -- u32
  // [count, done] at kWsDeoptOff (zero between batches), idx[n] past the tier-1 slots. The
  // compiled kernel appends the packet index of every lane that deoptimized (status kStDeopt: no
  // outputs, not counted); then the general interpreter runs with deopt_pass = 1 over
  // idx[0 .. count) (outputs at those indices), and its last workgroup zeroes count and done.
  // deopt_pass = 2 on a compiled store-mode launch that no pass follows (StackPlan::no_deopt): a
  // lane that still leaves is not listed but gets status EBPF_ST_JIT (the proof failed).
  uint32_t* deopt;
  uint32_t* deopt_idx;
  uint32_t deopt_pass;
  // EBPF_BATCH_WRITEBACK on the general interpreter's tier 1 (the deopt pass included): a lane that
  // ends EBPF_ST_OK stores its image's bytes [0, len) -- xdp_md: [8, 8 + len) -- back to its
  // packet (the compiled store kernels' write-back variant does it in its own code, jit.cpp).
  // (In the padding behind deopt_pass: the struct's layout, which the compiled statements read
  // by offset, is unchanged.)
  uint32_t writeback;
  // store mode on the var tile loop: per packet its image's bytes [64, 128) once it stores there
  // (u8[n][64] + 16 in the workspace past deopt_idx; jit.cpp ovf_fill), else null
  uint8_t* ovf;
};

constexpr int kTraceSlots = 16;
constexpr uint64_t kTraceWaves = 1 << 16;
constexpr int kTraceRing = 4;  // launches kept (consecutive launches' gaps)

// Bytes of tier-1 scratch per wave slot: lane-interleaved image dwords + call stack.
__host__ __device__ inline uint64_t tier1_slot_bytes(uint32_t mem_size) {
  return (uint64_t)((mem_size + 3) / 4 + kCallDepth) * kWave * 4;
}

// Programs this short with no back edge do a fixed, tiny amount of work per tile.
constexpr uint32_t kTinyUops = 8;

// Grid size on the current device. Tier 0 and DAG: one tile (64 packets) per wave, so the hardware
// dispatcher balances divergent tiles, except `tiny` programs, which get every resident wave
// slot once (grid-stride) so per-workgroup fixed costs are paid once per slot. Tier 1:
// balanced persistent waves (bounds the per-wave image scratch).
int interp_grid(int kind, uint32_t n_uops, bool tiny, uint64_t n_tiles, int* grid_out);

// Length-binned lane packing for the loop-mode tile kernel (offsets + lens layouts): fills
// perm[n] with the packet indices grouped by ceil(len / 128), so a tile's lanes run loops of
// similar trip counts. Two kernels on `stream` (histogram, scatter); bins start zeroed.
hipError_t launch_binning(const uint16_t* lens, uint64_t n, uint32_t* wgc, uint32_t* perm,
                          hipStream_t stream);

// xdp_md calling convention: stage image i = [xdp_md {8, 8 + len}][packet][...] for every packet
// into dst (16-byte aligned slots, packed in workgroup order); writes the staged offsets and
// lengths (8 + len). Images longer than mem_size are not copied (the batch faults them
// ST_BADPKT from the length alone). cursor: a zeroed u64.
hipError_t launch_xdp_stage(const uint8_t* frames, const uint32_t* offsets, const uint16_t* lens,
                            uint64_t stride, uint64_t n, uint32_t mem_size, uint8_t* dst,
                            uint32_t* doffs, uint16_t* dlens, unsigned long long* cursor,
                            hipStream_t stream);

// What of a batch's layout picks its kernel: everything launch_kernel_id reads of a batch. Taken
// from the batch's pointers (batch_layout), or stated outright for a batch whose arrays do not
// exist yet (host.cpp: the staged form of an xdp_md batch, whose offsets and lengths the library
// writes into its 16-byte aligned workspace).
struct BatchLayout {
  bool offsets = false, lens = false;  // the arrays are present
  bool offsets4 = true, lens4 = true;  //   ... and 4-byte aligned (true when absent)
  bool slots16 = false;                // frames and stride are both 16-byte aligned
  bool mem_out = false;                // the final images are an output
  bool xdp = false;                    // xdp_md in place (LaunchArgs::xdp)
  uint64_t stride = 0;
  uint64_t n_tiles = 0;
};
inline BatchLayout batch_layout(const uint8_t* frames, const uint32_t* offsets,
                                const uint16_t* lens, uint64_t stride, uint64_t n_tiles,
                                bool mem_out, bool xdp) {
  BatchLayout l;
  l.offsets = offsets != nullptr;
  l.lens = lens != nullptr;
  l.offsets4 = ((uintptr_t)offsets & 3) == 0;
  l.lens4 = ((uintptr_t)lens & 3) == 0;
  l.slots16 = (((uintptr_t)frames | (uintptr_t)stride) & 15) == 0;
  l.mem_out = mem_out;
  l.xdp = xdp;
  l.stride = stride;
  l.n_tiles = n_tiles;
  return l;
}

// Whether a layout is the fixed-slot one (stride layout, 16-byte aligned slots of >= 64 bytes, no
// lengths, no image output).
bool launch_fixed_layout(const BatchLayout& l);

// The EBPF_KERNEL_* id of the kernel that runs a batch of layout l: kind and n_uops of the
// program's table, jit its compiled kernels (null: interpreted), stack: a memory tier 0.5 batch.
// The one place that decides between the compiled kernels; launch_interp runs the id it is given.
int launch_kernel_id(int kind, uint32_t n_uops, const BatchLayout& l, const JitFns* jit, bool stack);

// dst[0..7] += src[0..7] on `stream` (one tiny kernel).
hipError_t launch_counters_add(const uint64_t* src, uint64_t* dst, hipStream_t stream);

// Enqueue kernel `id` (launch_kernel_id's answer for this batch) on `stream`; with counters, its
// last workgroup folds the shards into them. jit: the program's compiled kernels (the JIT_* ids).
// grid: interp_grid's; the compiled kernels size their own from their occupancy.
hipError_t launch_interp(int id, const LaunchArgs& a, int grid, hipStream_t stream,
                         const JitFns* jit = nullptr);

// ---- verdict queues and the packet gather (queues.hip) ----
constexpr int kQBlock = 256;             // 4 waves per workgroup
constexpr int kQWaves = kQBlock / kWave;
constexpr int kQClasses = 7;             // EBPF_NQUEUES
constexpr int kQSlots = 8;               // counts are kept 8 to a row (slot 7 is zero)
constexpr uint32_t kQRange = 4096;       // a workgroup's packets: a whole number of these, one
                                         // while the grid is not capped (each wave a quarter)
constexpr int kQMaxWgs = 1024;           // queues grid cap (a larger batch: longer ranges)
constexpr uint32_t kGTile = 256;         // gather: queue positions per workgroup pass (one a thread)
constexpr int kGMaxWgs = 1024;           // gather grid cap (a longer queue: several tiles in order)
// workspaces: [workgroup counts u32[kQMaxWgs][8]][wave counts u32[kQMaxWgs][4][8]]; the gather's
// workgroup byte sums u64[kGMaxWgs]. Neither needs zeroing: every word read was written first.
constexpr uint64_t kQWsWaveOff = (uint64_t)kQMaxWgs * kQSlots * 4;
constexpr uint64_t kQWsBytes = kQWsWaveOff + (uint64_t)kQMaxWgs * kQWaves * kQSlots * 4;
constexpr uint64_t kGWsBytes = (uint64_t)kGMaxWgs * 8;

// index[n] = the packet numbers stably partitioned by verdict class, count[7] = the class sizes
// (include/ebpf_emu.h ebpf_verdict_queues). Two kernels on `stream`; n >= 1.
hipError_t launch_queues(const uint8_t* verdict, uint64_t n, uint32_t* index, uint32_t* count,
                         uint8_t* ws, hipStream_t stream);

struct GatherArgs {  // ebpf_gather_desc, checked (cap = min(out_bytes, 2^32 - 1))
  const uint8_t* frames;
  const uint32_t* offsets;
  const uint16_t* lens;
  uint64_t stride;
  uint64_t n;
  const uint32_t* index;
  const uint32_t* count;
  uint32_t queue;
  uint32_t align;
  uint8_t* out_frames;
  uint64_t cap;
  uint32_t* out_offsets;
  uint16_t* out_lens;
  uint32_t* out_total;
  unsigned long long* wsum;  // workspace: u64[grid]
};
// Two kernels on `stream` (include/ebpf_emu.h ebpf_gather).
hipError_t launch_gather(const GatherArgs& g, hipStream_t stream);

// ---- the scatter: a gathered queue's packets and results put back (queues.hip)
struct ScatterArgs {  // ebpf_scatter_desc, checked: a result pair is both set or both null, the
                      // src_ packet arrays are set with frames, cap >= 1
  const uint32_t* index;
  const uint32_t* count;
  const uint32_t* total;
  uint32_t queue;
  uint32_t cap;
  const uint8_t* src_frames;
  uint64_t src_bytes;
  const uint32_t* src_offsets;
  const uint16_t* src_lens;
  const uint8_t* src_verdict;
  const uint8_t* src_status;
  const uint64_t* src_r0;
  uint8_t* frames;
  const uint32_t* offsets;
  const uint16_t* lens;
  uint64_t stride;
  uint64_t n;
  uint8_t* verdict;
  uint8_t* status;
  uint64_t* r0;
};
// One kernel on `stream`, its grid sized from cap as the gather's is from n (kGTile, kGMaxWgs).
hipError_t launch_scatter(const ScatterArgs& s, hipStream_t stream);

// ---- the pcap gather: a queue written out as a classic libpcap stream (queues.hip, DESIGN.md
// §3.40). Its workspace, per workgroup of the capped grid: [record bytes u64][records u32][bytes of
// the first record u32]; no zeroing, every word read was written first.
constexpr uint64_t kPWsCntOff = (uint64_t)kGMaxWgs * 8;
constexpr uint64_t kPWsFirstOff = kPWsCntOff + (uint64_t)kGMaxWgs * 4;
constexpr uint64_t kPWsBytes = kPWsFirstOff + (uint64_t)kGMaxWgs * 4;
constexpr uint32_t kPcapSrcRecords = 1, kPcapSwapped = 2;  // EBPF_PCAP_SRC_RECORDS / _SWAPPED

struct PcapArgs {  // ebpf_pcap_gather_desc, checked (cap = min(out_bytes, 2^32 - 1)); the source
                   // batch and the queue under GatherArgs' names (g_queue / g_packet read both)
  const uint8_t* frames;
  const uint32_t* offsets;
  const uint16_t* lens;
  uint64_t stride;
  uint64_t n;
  const uint32_t* index;
  const uint32_t* count;
  uint32_t queue;
  uint32_t flags;
  uint32_t snaplen;
  uint32_t hdr[6];      // the global header's 24 bytes
  const uint32_t* ts;   // optional u32[n][2]
  uint8_t* out;
  uint64_t cap;
  uint32_t* out_offsets;  // optional
  uint16_t* out_lens;     // optional
  uint32_t* out_total;
  unsigned long long* wsum;  // workspace: u64[grid], u32[grid], u32[grid]
  uint32_t* wcnt;
  uint32_t* wfirst;
};
// Two kernels on `stream` (include/ebpf_emu.h ebpf_pcap_gather); n >= 1.
hipError_t launch_pcap_gather(const PcapArgs& p, hipStream_t stream);

// ---- RSS flow steering (steer.hip) ----
constexpr int kRssBlock = 256;            // one lane per packet
constexpr int kRssMaxWgs = 2048;          // hash grid cap (a larger batch: several passes)
constexpr int kRssKeyBytes = 40;
constexpr int kRssWindows = 288;          // input bits of the longest input (36 bytes)
constexpr uint32_t kRssTypes = 63;        // every EBPF_RSS_* bit

struct RssArgs {  // ebpf_rss_desc, checked
  const uint8_t* frames;
  const uint32_t* offsets;
  const uint16_t* lens;
  uint64_t stride;
  uint64_t n;
  uint32_t types;
  uint32_t* hash;
  uint8_t* type;  // optional
  // win[i] = key bits [i, i + 32) as a number: what input bit i XORs into the hash. Uniform over
  // the launch, read by constant index: the kernel holds them in scalar registers.
  uint32_t win[kRssWindows];
};
// One kernel on `stream` (include/ebpf_emu.h ebpf_rss_hash); n >= 1.
hipError_t launch_rss_hash(const RssArgs& r, hipStream_t stream);

constexpr int kSBlock = 256;              // steer: 4 waves per workgroup
constexpr int kSWaves = kSBlock / kWave;
constexpr int kSClasses = 64;             // EBPF_STEER_MAX_QUEUES: counts are kept 64 to a row
constexpr int kSReta = 128;               // EBPF_STEER_MAX_RETA
constexpr uint32_t kSRange = 4096;        // a workgroup's keys: a whole number of these, one while
                                          // the grid is not capped (each wave a quarter)
constexpr int kSMaxWgs = 1024;            // steer grid cap (a larger batch: longer ranges)
// workspace: [workgroup counts, then bases, u32[kSMaxWgs][64]][wave counts u32[kSMaxWgs][4][64]].
// No zeroing: every word read was written first.
constexpr uint64_t kSWsWaveOff = (uint64_t)kSMaxWgs * kSClasses * 4;
constexpr uint64_t kSWsBytes = kSWsWaveOff + (uint64_t)kSMaxWgs * kSWaves * kSClasses * 4;

struct SteerArgs {  // ebpf_steer's arguments, checked
  const uint32_t* key;
  uint64_t n;
  uint32_t nq;
  uint32_t mask;   // reta_len - 1
  uint32_t bits;   // class bits that can be set: ceil(log2(nq))
  uint32_t* index;
  uint32_t* bounds;
  uint32_t* wgc;   // workspace
  uint32_t* wvc;
  uint8_t reta[kSReta];  // entries < nq <= 64
};
// Three kernels on `stream` (include/ebpf_emu.h ebpf_steer); n >= 1.
hipError_t launch_steer(const SteerArgs& s, hipStream_t stream);

// ---- checksum offload (csum.hip) ----
// One wave per workgroup: the LDS arrays are a wave's own, so the two barriers of a pass couple no
// wave to another one's longer block list.
constexpr int kCsBlock = 64;              // one lane per packet to parse
constexpr int kCsWaves = kCsBlock / kWave;
constexpr int kCsMaxWgs = 8192;           // grid cap (a larger batch: several passes)
constexpr uint32_t kCsWhat = 7;           // every EBPF_CSUM_IPV4_HDR / _TCP / _UDP bit

struct CsumArgs {  // ebpf_csum_desc, checked
  uint8_t* frames;
  const uint32_t* offsets;
  const uint16_t* lens;
  uint64_t stride, n;
  uint32_t what;
  uint32_t queue_mask;     // the caller's; not looked at when verdict == nullptr
  const uint8_t* verdict;  // optional
  uint8_t* status;         // optional (fill)
};
// One kernel on `stream` (include/ebpf_emu.h ebpf_csum_verify / ebpf_csum_fill); n >= 1.
hipError_t launch_csum(const CsumArgs& c, bool fill, hipStream_t stream);

}  // namespace ebpfemu
