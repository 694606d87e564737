/*
 * ebpf_emu.h — C ABI of libebpfemu.so, the MI355X-native batched eBPF/XDP interpreter.
 *
 * Drop-in boundary for b1tg/ebpf-emu's load-program / run(packet) -> verdict surface
 * (reference snapshot 2024-12-20). Each entry point names the reference interface it
 * replaces. Plain pointers and sizes only; no torch / C++ types. Every call returns an int:
 * 0 = OK, < 0 = EBPF_E* (no aborts). Per-packet faults go to a status array instead of the
 * reference's process-killing panics.
 *
 * Threading: a loaded program is immutable and may be shared across host threads and
 * devices. Batch launches are asynchronous and ordered on the caller's HIP stream. The library's
 * per-(device, stream) workspace (counter shards, the deopt list, the overflow images) is found
 * and grown under a lock and never freed while the library is loaded, so host threads may launch
 * concurrently; but launches on the SAME stream from two threads must be ordered by the caller
 * (as any work on one HIP stream): the workspace is reused by every launch on that stream.
 */
#ifndef EBPF_EMU_H
#define EBPF_EMU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ebpf_prog ebpf_prog;
typedef struct ihipStream_t* ebpf_stream_t; /* == hipStream_t */

/* ---- error codes (load-time rejects mirror the reference's decode panics) ---- */
#define EBPF_OK             0
#define EBPF_EINVAL        (-1)  /* bad argument */
#define EBPF_ELEN          (-2)  /* image not a whole number of 8-byte words (ins.rs:66-67) */
#define EBPF_EREG          (-3)  /* register nibble >= 12 (ins.rs:32) */
#define EBPF_EOP           (-4)  /* ALU/JMP op > 0xd (ins.rs:251,257) */
#define EBPF_EMODE         (-5)  /* LS mode 0xe0 (ins.rs:187) or invalid discriminant 0x80/0xa0 */
#define EBPF_ELDDW         (-6)  /* wide instruction missing its second word (ins.rs:112) */
#define EBPF_ELDDW_OVF     (-7)  /* imm64 fold overflow (debug-build panic, ins.rs:112) */
#define EBPF_EHEX          (-8)  /* malformed hex (ins.rs:46-74 error strings) */
#define EBPF_ENOMEM        (-9)
#define EBPF_EHIP          (-10) /* a HIP runtime call failed */
#define EBPF_ETOOBIG       (-11) /* program beyond the device limit (EBPF_MAX_INSNS) */
#define EBPF_ERCCL         (-12) /* an RCCL call failed */
#define EBPF_EPCAP         (-13) /* not a classic pcap capture, or a truncated record */
#define EBPF_EJIT          (-14) /* the program compiler failed (amd_comgr assembler/linker) */

/* ---- per-packet status (u8) ---- */
#define EBPF_ST_OK          0  /* exit with empty frame stack or pc past the end (emu.rs:49,277) */
#define EBPF_ST_MEM         1  /* memory bounds / address-overflow panic (mmu.rs:16,26; emu.rs:344) */
#define EBPF_ST_MEM_UB      2  /* first byte in bounds, tail not: UB in the reference (mmu.rs:23-30) */
#define EBPF_ST_INSN        3  /* runtime instruction panic (emu.rs:206,270,336,339,351,421,438) */
#define EBPF_ST_ARITH       4  /* debug-build overflow panic (emu.rs:162,268,393,427) */
#define EBPF_ST_STEPS       5  /* step budget exhausted (reference: no limit, hangs; emu.rs:452) */
#define EBPF_ST_CALLDEPTH   6  /* frame stack deeper than EBPF_MAX_CALL_DEPTH */
#define EBPF_ST_BADPKT      7  /* packet longer than the memory image (main.rs:20-21) */
#define EBPF_ST_JIT         8  /* a compiled kernel's load-time proof did not hold for this packet
                                 (a library bug, never expected: the packet was not run) */

/* ---- verdict byte (xdp_action, xdp.rs:3-9) ---- */
#define EBPF_XDP_ABORTED    0
#define EBPF_XDP_DROP       1
#define EBPF_XDP_PASS       2
#define EBPF_XDP_TX         3
#define EBPF_XDP_REDIRECT   4
#define EBPF_VERDICT_OTHER  0xFE /* r0 >= 5 */
#define EBPF_VERDICT_FAULT  0xFF /* status != OK */

/* ---- counters[EBPF_NCOUNTERS] (accumulated, u64) ---- */
#define EBPF_CNT_R0_0       0   /* ... EBPF_CNT_R0_0 + 4: r0 == 0..4 */
#define EBPF_CNT_OTHER      5   /* r0 >= 5 */
#define EBPF_CNT_FAULT      6   /* status != OK */
#define EBPF_CNT_RETIRED    7   /* eBPF instructions executed */
#define EBPF_NCOUNTERS      8

#define EBPF_MAX_INSNS      65536  /* decoded instructions per program */
#define EBPF_MAX_CALL_DEPTH 64
/* ebpf_batch.flags: run on the general interpreter even when the program qualifies for the
 * forward-jump fast path (differential testing; results are identical by contract). */
#define EBPF_BATCH_GENERIC 1u
/* ebpf_batch.flags: the xdp_md calling convention (xdp.rs:16-20, struct xdp_md { u32 data;
 * u32 data_end; }). Each packet's memory image becomes [xdp_md][packet][zeros]: data = 8,
 * data_end = 8 + len at image offsets 0 and 4, the packet at offset 8, so r1 (= 0) is the ctx
 * pointer, standard XDP programs run unchanged, and r2 = 8 + len (main.rs:18-29 gives r2 the
 * image length). This is exactly the image the reference executes when main.rs is handed the
 * ctx-prefixed bytes. The compiled forward kernels (and the tile interpreter on offsets / lens
 * layouts) run such a batch in place: the ctx is synthesised in each packet's LDS window and the
 * packet read 8 bytes further on, with no extra pass over the frames. Other kernels (loop
 * programs, the general interpreter) run images the library stages in the workspace first.
 * Requires mem_size <= 65528. */
#define EBPF_BATCH_XDP_MD  2u
/* ebpf_batch.flags: run a compiled program (ebpf_prog_compile) on the tile interpreter instead
 * (differential testing; results are identical by contract). */
#define EBPF_BATCH_NO_JIT  4u
/* ebpf_batch.flags: write each packet's rewrite back in place, as an XDP program rewrites the
 * buffer the NIC then sends. `frames` is WRITTEN. Once the batch has completed on its stream:
 *   - a packet with status EBPF_ST_OK holds the final image's bytes [0, len) (with
 *     EBPF_BATCH_XDP_MD: image bytes [8, 8 + len); stores into the ctx words go nowhere);
 *   - a packet with any other status (a fault, EBPF_ST_STEPS, EBPF_ST_BADPKT, EBPF_ST_JIT) holds
 *     exactly its input bytes: a run is transactional per packet;
 *   - no byte outside the packets is written: not the gaps between offsets-layout packets, not the
 *     bytes of a stride slot past lens[i]; stores at image addresses >= len (the stack, a trailer
 *     past a short packet) are dropped. In the stride layout without lens, len = stride.
 * The caller's packets must not overlap (not checked). Every other output is bit-identical to the
 * same batch without the flag, and out->mem may be requested as well. A program without stores
 * runs the same kernel with and without the flag. (new: no reference counterpart; the reference
 * runs one packet and prints r0) */
#define EBPF_BATCH_WRITEBACK 8u
#define EBPF_DEFAULT_MEM    1024   /* main.rs:16 */
#define EBPF_DEFAULT_R10    512    /* main.rs:31 */
#define EBPF_DEFAULT_STEPS  (1ull << 22)

/* Batch descriptor. All pointers are DEVICE pointers on the device the stream belongs to.
 * Memory image per packet (main.rs:14-31 layout, sizes as launch parameters): mem_size zeroed
 * bytes, packet at [0,len), r1 = 0, r2 = len, r10 = r10, other registers 0. */
typedef struct ebpf_batch {
  const uint8_t* frames;    /* packet bytes (const: read only -- except with EBPF_BATCH_WRITEBACK,
                               which writes the packets' rewritten bytes back through it) */
  const uint32_t* offsets;  /* packet i at frames + offsets[i]; NULL => frames + i*stride */
  const uint16_t* lens;     /* packet i length; NULL => stride */
  uint64_t stride;          /* bytes between packets in the stride layout, where frames must hold
                               n * stride bytes (every slot whole, as in a ring of fixed slots) */
  uint64_t n;               /* packets */
  uint32_t mem_size;        /* bytes of the per-packet memory image, 0..2^24 (any length: Mmu.memory
                               is a Vec<u8>, mmu.rs:2-4) */
  uint32_t flags;           /* 0, or EBPF_BATCH_GENERIC | EBPF_BATCH_XDP_MD | EBPF_BATCH_NO_JIT |
                               EBPF_BATCH_WRITEBACK */
  uint64_t r10;             /* initial r10 (stack top) */
  uint64_t max_steps;       /* per-packet step budget, 1..; faults EBPF_ST_STEPS beyond */
  void* workspace;          /* optional device scratch of ebpf_workspace_bytes() bytes, ZEROED before its
                               first use and then reused as is (each batch leaves its counter
                               shards at zero); one workspace per stream; NULL => library-owned
                               per (device, stream) */
  uint64_t workspace_bytes;
  const uint64_t* init_regs; /* optional device u64[11]: initial r0..r10 for every packet, replacing
                                the main.rs layout (Emu.state.regs set by the caller, emu.rs:14-17) */
  const uint32_t* init_fp;  /* optional device u32[init_fp_len]: the initial frame stack of every
                               packet, bottom first (Emu.fp is pub, emu.rs:26; an EXIT pops its top,
                               emu.rs:273-279). A batch with one runs on the general interpreter */
  uint32_t init_fp_len;     /* 0..EBPF_MAX_CALL_DEPTH */
} ebpf_batch;

/* Outputs (device pointers; any may be NULL). */
typedef struct ebpf_batch_out {
  uint8_t* verdict;   /* u8[n]: r0 < 5 ? r0 : 0xFE; 0xFF on fault */
  uint64_t* r0;       /* u64[n]: raw r0 (two's complement of the reference's i64, main.rs:43);
                         for a packet with status != EBPF_ST_OK (the reference panics) r0 is the
                         register at the fault, except on a stack-slot promoted program's kernel,
                         where it is unspecified */
  uint8_t* status;    /* u8[n]: EBPF_ST_* */
  uint64_t* counters; /* u64[EBPF_NCOUNTERS], ADDED to (not overwritten) */
  uint8_t* mem;       /* u8[n][mem_size]: final memory image per packet (Emu.state.mmu.memory) */
  uint64_t* regs;     /* u64[n][11]: final r0..r10 per packet (Emu.state.regs) */
  uint32_t* fp;       /* u32[n][EBPF_MAX_CALL_DEPTH]: final frame stack per packet, bottom first
                         (Emu.fp; non-empty when a program falls off its end inside a call) */
  uint8_t* fp_len;    /* u8[n]: its depth */
} ebpf_batch_out;

/* Fill a batch descriptor with the reference harness defaults (mem 1024, r10 512). */
void ebpf_batch_init(ebpf_batch* b);

/* Load a program from its little-endian byte image.
 * Replaces ins::u64s_to_instructions (ins.rs:96-119) + Instruction::from (ins.rs:121-132) +
 * Code::from (ins.rs:148-173); a decode panic becomes an EBPF_E* return. On error,
 * *bad_word (if non-NULL) receives the index of the offending 8-byte word. */
int ebpf_prog_load(const uint8_t* code, size_t nbytes, ebpf_prog** out, size_t* bad_word);

/* Load from hex text. Replaces ins::hexs_to_instructions (ins.rs:91-94): whitespace is
 * removed, the rest parsed as 16-digit big-endian u64 words (ins.rs:60-74). */
int ebpf_prog_load_hex(const char* hex, ebpf_prog** out, size_t* bad_word);

void ebpf_prog_free(ebpf_prog* prog);

/* Number of decoded instructions (a wide lddw counts once, ins.rs:107-116). */
size_t ebpf_prog_len(const ebpf_prog* prog);

/* Copy decoded instruction i out as the reference's Instruction fields (ins.rs:37-45). */
int ebpf_prog_insn(const ebpf_prog* prog, size_t i, int32_t* imm, int64_t* imm64, int16_t* off,
                   uint8_t* src, uint8_t* dst, uint8_t* code);

/* Memory tier the device path uses for this program: 0 = read-only packet window (no stores,
 * no calls), 1 = general per-packet image in device workspace. */
int ebpf_prog_tier(const ebpf_prog* prog);

/* 1 when the program (memory tier 0, every jump forward, <= EBPF_MAX_COMPILED_UOPS micro-ops)
 * runs on the forward-jump fast path -- for batches with max_steps >= its length and without
 * EBPF_BATCH_GENERIC; past 256 micro-ops only compiled (ebpf_prog_compile), not with
 * EBPF_BATCH_NO_JIT -- else 0; -1 for NULL. */
int ebpf_prog_forward_only(const ebpf_prog* prog);

/* Memory tier 0.5: the bytes of the stack window [r10 - k, r10) of a program whose memory writes
 * are ST/STX/ATOMIC at r10 + c (c known at load time, all in the window; atomics 4-aligned), or
 * ST/STX into the packet's first 64 bytes at load-time constant addresses (then every other load
 * must be a constant-address or stack-window one); forward jumps only, no CALL, <= 62 micro-ops.
 * Such a program keeps the window (and the stored packet bytes) in registers of the compiled
 * fixed-slot kernel, for batches in the fixed-slot layout with the main.rs register layout whose
 * window lies past every packet byte and inside the image (r10 % 4 == 0); other batches run it
 * on the general interpreter. A program with packet stores only reports a 4-byte window.
 * 0 = not such a program; -1 for NULL. */
int ebpf_prog_stack_window(const ebpf_prog* prog);

/* Store mode: ST/STX through a register whose value is not known at load time (a packet pointer
 * behind a variable-length header; reference emu.rs:354-372). Such a program runs on the compiled
 * fixed-slot kernel (fixed slots) or the var kernels with its header window in LDS; a lane whose access leaves the image bytes the kernel
 * holds is re-run by the general interpreter after the launch (the deopt pass). 0 = not store
 * mode, 1 = store mode with the deopt pass, 2 = store mode proven at load time to need no pass
 * for main.rs-layout batches (no lane can leave; a lane that did would fault EBPF_ST_JIT); -1 for
 * NULL. */
int ebpf_prog_store_mode(const ebpf_prog* prog);

/* Micro-ops (after local calls are flattened into one copy per frame stack) of the longest
 * program the compiler takes; longer programs run on the general interpreter. */
#define EBPF_MAX_COMPILED_UOPS 4096

/* Compile the program to gfx950 machine code now, if it is one the tile kernels run (memory tier
 * 0): straight-line code in pc order with direct register operands, replacing the interpreter's
 * dispatch, for programs of <= EBPF_MAX_COMPILED_UOPS micro-ops. Forward-only programs get the forward kernels
 * (batches with max_steps >= the program length); every such program also gets the loop kernel
 * (back edges, or a step budget that can bind: the exact budget of the reference's step count). Needs no
 * GPU; done implicitly by the first upload. Returns 1 = compiled, 0 = not such a program,
 * EBPF_EJIT on a compiler failure (ebpf_prog_jit_error says why; EBPF_BATCH_NO_JIT runs a compiled
 * program's batch interpreted). */
int ebpf_prog_compile(ebpf_prog* prog);

/* The compiled program's gfx950 assembly (variant 0: forward-only, batches with init_regs; 1:
 * forward-only, the main.rs register layout, whose constant-address loads are resolved; 2: the
 * loop-program kernel; 3: forward-only for xdp_md batches; 4: the stack-slot promoted loop
 * program; 5, 6: the loop program for xdp_md batches, staged / in place; 7: the write-back
 * variant -- variant 1 of a stack-window program with packet stores, followed by the stores of
 * the rewritten packet bytes, EBPF_BATCH_WRITEBACK; compiled by the first request for it or the
 * first batch with the flag), for inspection: copies up to cap bytes (NUL-terminated) and sets *len to
 * the full length. EBPF_EINVAL if that variant is not compiled. */
int ebpf_prog_jit_asm(ebpf_prog* prog, int variant, char* buf, size_t cap, size_t* len);

/* Why the program is not (wholly) compiled: compiles it first, then copies up to cap bytes
 * (NUL-terminated) of the reason -- the compiler's or assembler's error, or why the program is
 * not one the compiler takes -- and sets *len to its length; "" when every variant compiled.
 * Once the write-back variant (7) has been asked for and failed, its reason is appended: such a
 * program's EBPF_BATCH_WRITEBACK batches run the general interpreter (ebpf_batch_kernel says so).
 * (new: no reference counterpart; diagnostics for ebpf_prog_compile) */
int ebpf_prog_jit_error(ebpf_prog* prog, char* buf, size_t cap, size_t* len);

/* Device scratch a batch needs (counter shards; tier 1 adds per-wave memory images). */
uint64_t ebpf_workspace_bytes(const ebpf_prog* prog, const ebpf_batch* batch, int device);

/* Copy the device micro-op table to `device` now (otherwise done on first run there).
 * Synchronous; call it before capturing ebpf_run_batch into a HIP graph. */
int ebpf_prog_upload(ebpf_prog* prog, int device);

/* Run a batch on the device owning `stream` (NULL = the current device's null stream).
 * Replaces, per packet, Emu::default() + Mmu setup + Emu::run() + reading state.regs[0]
 * (main.rs:14-43, emu.rs:30-45,452-458). Asynchronous, stream-ordered: one interpreter
 * kernel; with out->counters, its last workgroup folds the per-shard sums into them. */
int ebpf_run_batch(ebpf_prog* prog, const ebpf_batch* batch, const ebpf_batch_out* out,
                   ebpf_stream_t stream);

/* The kernel ebpf_run_batch runs for this batch and outputs on `device`: the kernel id of the
 * plan ebpf_run_batch executes, made by the same function from the same inputs (host.cpp
 * plan_batch; the program is uploaded to the device first, so it needs that device). One of
 * EBPF_KERNEL_*, or < 0 = EBPF_E*. */
#define EBPF_KERNEL_GENERAL_T0 0  /* interp_kernel, memory tier 0 (read-only packet window) */
#define EBPF_KERNEL_GENERAL_T1 1  /* interp_kernel, memory tier 1 (per-packet images in scratch) */
#define EBPF_KERNEL_DAG        2  /* dag_kernel: forward-only programs of 63..256 micro-ops */
#define EBPF_KERNEL_TILE       3  /* tile interpreter, forward-only programs */
#define EBPF_KERNEL_TILE_LOOP  4  /* tile interpreter, loop mode */
#define EBPF_KERNEL_JIT_FIXED  5  /* compiled program, fixed-slot layout (ebpf_tile_jit_fixed) */
#define EBPF_KERNEL_JIT_VAR    6  /* compiled program, other layouts (ebpf_tile_jit_var) */
#define EBPF_KERNEL_JIT_LOOP   7  /* compiled loop program (ebpf_tile_jit_loop) */
#define EBPF_KERNEL_JIT_STACK  8  /* compiled stack-window program (memory tier 0.5, fixed slots;
                                    store mode included; with EBPF_BATCH_WRITEBACK its write-back
                                    variant, as EBPF_KERNEL_JIT_VARL_STACK's -- a write-back batch
                                    that would run EBPF_KERNEL_JIT_VAR_STACK runs
                                    EBPF_KERNEL_GENERAL_T1 instead) */
#define EBPF_KERNEL_JIT_VAR_STACK 9  /* compiled stack-window program, other layouts
                                        (ebpf_tile_jit_var_stack) */
#define EBPF_KERNEL_JIT_LOOP_STACK 10 /* compiled stack-window loop program
                                         (ebpf_tile_jit_loop_stack) */
#define EBPF_KERNEL_JIT_VARL   11 /* compiled program, offsets + lens batches: the var tile loop
                                    (ebpf_tile_jit_varl; offsets and lens 4-byte aligned, no
                                    final images) */
#define EBPF_KERNEL_JIT_VARL_STACK 12 /* the var tile loop for stack-window programs
                                         (ebpf_tile_jit_varl_stack; store mode included) */
#define EBPF_KERNEL_JIT_FIXED_OCC 13 /* compiled forward program, fixed-slot layout: the kernel's
                                        occupancy variant (ebpf_tile_jit_fixed_occ; every program
                                        whose code fits it, not xdp_md, no stack window) */
int ebpf_batch_kernel(ebpf_prog* prog, const ebpf_batch* batch, const ebpf_batch_out* out,
                      int device);

/* Whether ebpf_run_batch stages this EBPF_BATCH_XDP_MD batch's images (one copy kernel writing
 * [ctx][packet] per packet into the workspace before the program's kernel, xdp.rs:16-20) on
 * `device`, read from the same plan as ebpf_batch_kernel's answer: 1 staged, 0 in place (or not
 * an xdp_md batch), < 0 = EBPF_E*. */
int ebpf_batch_staged(ebpf_prog* prog, const ebpf_batch* batch, const ebpf_batch_out* out,
                      int device);

/* Multi-GPU: shard s runs on devices[s] / streams[s] (distinct devices); the shards' counters are
 * summed with one RCCL all-reduce over xGMI, and the global totals of this call are ADDED to
 * every outs[s].counters (accumulated as in ebpf_run_batch, never overwritten; the per-shard sums
 * go through 64 bytes of the shard's workspace first -- batches[s].workspace, or the
 * library-owned one of (device, stream)). Shards are independent (no data-path exchange).
 * Requires counters in every out. A failing call leaves every caller counter untouched. Returns
 * after enqueueing (asynchronous on each stream, so calls on the same streams are ordered). */
int ebpf_run_batch_multi(ebpf_prog* prog, int nshards, const int* devices,
                         const ebpf_batch* batches, const ebpf_batch_out* outs,
                         ebpf_stream_t const* streams);

/* Host ingestion (the path starts in host memory, "a pcap buffer or NIC ring").
 * Index a classic libpcap capture held in host memory (magic a1b2c3d4 / a1b23c4d, either byte
 * order): offsets[i] / lens[i] = the byte offset and captured length of record i's packet
 * within buf. A device copy of the same bytes plus these arrays is an offsets + lens batch, so
 * the capture runs unmodified (no repacking). Records are indexed in file order; at most cap of
 * them (offsets/lens may be NULL with cap 0 to count). *n receives the number of records in
 * the buffer, *linktype the capture's link type (1 = Ethernet). Returns EBPF_EPCAP for a bad
 * header or a truncated record, EBPF_ETOOBIG for a record longer than 65535 bytes or a buffer
 * past 4 GiB (u32 offsets: index such a capture in pieces), EBPF_EINVAL when more than cap
 * records exist (the first cap are indexed). The reference reads its packet from argv
 * (main.rs:14-22); this replaces that per-packet input for whole captures. */
int ebpf_pcap_index(const uint8_t* buf, size_t nbytes, uint32_t* offsets, uint16_t* lens,
                    size_t cap, size_t* n, uint32_t* linktype);

/* ---- verdict queues and the packet gather: what a datapath does with a batch's verdicts ----
 * (new: no reference counterpart; the reference runs one packet and prints r0. The queues follow
 * the action enum, xdp.rs:3-9.) The calls (ebpf_scatter below included) are asynchronous and
 * ordered on `stream` as ebpf_run_batch is, make no host synchronisation, and allocate nothing
 * when a workspace is passed: run -> queues -> gather chains on one stream and none of the three
 * ever synchronises. The NEXT ebpf_run_batch takes its n from the host, though: running the
 * gathered batch costs one 8-byte read of out_total, the chain's only host round trip. */

/* Queue q holds the packets of verdict q for q = 0..4 (ABORTED, DROP, PASS, TX, REDIRECT);
 * queue 5 every other verdict byte but 0xFF (EBPF_VERDICT_OTHER; bytes 5..0xFD count here too);
 * queue 6 EBPF_VERDICT_FAULT -- the order of counters 0..6. */
#define EBPF_NQUEUES 7

/* Device scratch ebpf_verdict_queues needs for n packets (8-byte aligned; needs no zeroing). */
uint64_t ebpf_queues_workspace_bytes(uint64_t n);

/* The stable partition of the packet numbers 0..n-1 by queue. Once complete on the stream:
 * count[q] = packets in queue q; queue q is index[start_q .. start_q + count[q]) with start_q =
 * count[0] + ... + count[q-1]; inside a queue the packet numbers ascend (a flow's packets leave in
 * arrival order; the result is deterministic).
 * verdict: device u8[n] (any alignment); index: device u32[n]; count: device u32[EBPF_NQUEUES],
 * OVERWRITTEN. workspace: device scratch of ebpf_queues_workspace_bytes(n) bytes, one per stream;
 * NULL => library-owned per (device, stream), a buffer of its own (not the batch workspace).
 * n == 0 is valid: the counts are 0 and nothing else is written. Returns EBPF_ETOOBIG for
 * n > UINT32_MAX; EBPF_EINVAL, before any device call, for a NULL count, a NULL verdict or index
 * with n > 0, or a workspace that is too small. */
int ebpf_verdict_queues(const uint8_t* verdict, uint64_t n, uint32_t* index, uint32_t* count,
                        void* workspace, uint64_t workspace_bytes, ebpf_stream_t stream);

/* One queue's packets copied into a dense offsets + lens batch (itself the input of a next
 * ebpf_run_batch: out_frames / out_offsets / out_lens with n = out_total[0]). All pointers are
 * DEVICE pointers. */
typedef struct ebpf_gather_desc {
  const uint8_t* frames;    /* the source batch, as in ebpf_batch: packet i at frames + offsets[i], */
  const uint32_t* offsets;  /*   or frames + i*stride when NULL; */
  const uint16_t* lens;     /*   its length lens[i], or stride when NULL (then stride <= 65535) */
  uint64_t stride;
  uint64_t n;               /* packets in the source batch (<= UINT32_MAX) */
  const uint32_t* index;    /* ebpf_verdict_queues' index, u32[n] */
  const uint32_t* count;    /* its count[EBPF_NQUEUES], READ ON THE DEVICE (no host sync) */
  uint32_t queue;           /* 0..EBPF_NQUEUES-1 */
  uint32_t align;           /* power of two, 1..256: output packet j starts at a multiple of it */
  uint8_t* out_frames;      /* u8[out_bytes] */
  uint64_t out_bytes;       /* <= 4 GiB (u32 offsets) */
  uint32_t* out_offsets;    /* u32[n] */
  uint16_t* out_lens;       /* u16[n] */
  uint32_t* out_total;      /* u32[2], OVERWRITTEN: packets written, end byte of the last one */
  void* workspace;          /* optional scratch of ebpf_gather_workspace_bytes(n) bytes (8-byte
                               aligned, no zeroing); NULL => library-owned per (device, stream) */
  uint64_t workspace_bytes;
} ebpf_gather_desc;

uint64_t ebpf_gather_workspace_bytes(uint64_t n);

/* With m = count[queue] and s_j the j-th packet of that queue: out_lens[j] = len(s_j);
 * out_offsets[j] = the sum over i < j of alignup(len(s_i), align); out_frames[out_offsets[j] ..
 * + len) = the packet's bytes as they are in `frames` when the call runs on the stream (after an
 * EBPF_BATCH_WRITEBACK batch: the rewritten bytes). A zero-length packet gets an entry and no
 * bytes. Packet j is written iff out_offsets[j] + len <= out_bytes (and <= 2^32 - 1: the offsets
 * and the end byte are u32); the offsets ascend, so the written packets are a prefix, and
 * out_total = {packets written, out_offsets[last] + len(last)} ({0, 0} when none). Entries of
 * out_offsets / out_lens at or past the prefix, every byte at or past out_bytes and every byte at
 * or past alignup(out_total[1], align) are untouched; the padding between a packet's end and the
 * next multiple of align has unspecified content. Source and output must not overlap (not
 * checked). The grid is sized from n and m is read on the device. Returns EBPF_EINVAL, before any
 * device call, for a NULL descriptor or pointer (out_frames may be NULL with out_bytes 0), no
 * packet layout, queue >= EBPF_NQUEUES, align not a power of two in 1..256 or a workspace that is
 * too small; EBPF_ETOOBIG for out_bytes > 4 GiB or n > UINT32_MAX. */
int ebpf_gather(const ebpf_gather_desc* g, ebpf_stream_t stream);

/* The way back: a gathered queue's packets (as a second ebpf_run_batch left them, rewritten with
 * EBPF_BATCH_WRITEBACK perhaps) and that run's per-packet results, put back at the packets' own
 * numbers in the original batch. All pointers are DEVICE pointers; every src_ array and `frames`
 * is optional. */
typedef struct ebpf_scatter_desc {
  const uint32_t* index;       /* ebpf_verdict_queues' index, u32[n] */
  const uint32_t* count;       /* its count[EBPF_NQUEUES], READ ON THE DEVICE (no host sync) */
  const uint32_t* total;       /* optional u32[2]: the gather's out_total (total[0] is read) */
  uint32_t queue;              /* 0..EBPF_NQUEUES-1 */
  uint64_t cap;                /* HOST value (<= UINT32_MAX): entries present in the src_ arrays, an
                                  upper bound on the queue positions scattered; sizes the grid */
  const uint8_t* src_frames;   /* the dense side: the gather's out_frames, u8[src_bytes], */
  uint64_t src_bytes;          /*   <= 4 GiB, */
  const uint32_t* src_offsets; /*   its out_offsets, u32[cap], */
  const uint16_t* src_lens;    /*   its out_lens, u16[cap]; */
  const uint8_t* src_verdict;  /*   the second run's outputs: u8[cap] (any alignment), */
  const uint8_t* src_status;   /*   u8[cap] (any alignment), */
  const uint64_t* src_r0;      /*   u64[cap] */
  uint8_t* frames;             /* the destination batch, as in ebpf_batch and WRITTEN: packet i at */
  const uint32_t* offsets;     /*   frames + offsets[i], or frames + i*stride when NULL; its length */
  const uint16_t* lens;        /*   lens[i], or stride when NULL. frames == NULL: results only */
  uint64_t stride;
  uint64_t n;                  /* packets in the destination batch (<= UINT32_MAX) */
  uint8_t* verdict;            /* u8[n] (any alignment), u8[n] (any alignment), u64[n]: each is */
  uint8_t* status;             /*   written only when it and its src_ partner are both non-NULL */
  uint64_t* r0;
  void* workspace;             /* optional scratch of ebpf_scatter_workspace_bytes(cap) bytes */
  uint64_t workspace_bytes;
} ebpf_scatter_desc;

/* 0 today: destinations and source offsets are both given, so the one kernel needs no scratch. */
uint64_t ebpf_scatter_workspace_bytes(uint64_t cap);

/* With start = count[0] + ... + count[queue-1] and m = min(count[queue], cap, total ? total[0] :
 * UINT32_MAX) -- both clamped so that index is read inside index[0, n) only -- queue position
 * j < m belongs to destination packet d = index[start + j]. An entry is VALID when d < n and, with
 * `frames`, its source span lies inside the dense buffer: src_offsets[j] + src_lens[j] <=
 * src_bytes. Once the call has completed on the stream, for every valid entry:
 *   verdict[d] = src_verdict[j], status[d] = src_status[j], r0[d] = src_r0[j] (the pairs present);
 *   with L = min(src_lens[j], len(d)), len(d) = lens[d] or stride: bytes [0, L) of packet d =
 *   src_frames[src_offsets[j] .. + L). L == 0 writes no bytes; the results are still merged.
 * Nothing else is written: not the entries of verdict / status / r0 that are no d, not one byte of
 * `frames` outside those [0, L) -- the rest of a longer slot, the gap to the next packet, a
 * neighbour that abuts at any alignment (a packet's partial first and last 16-byte pieces are
 * stored with naturally aligned 1/2/4/8-byte stores, never by read-modify-write of a wider word)
 * -- and nothing at all for an entry that is not valid: a wrong index never becomes a wild store.
 * Reads of src_frames stay inside the aligned 16-byte blocks that hold a byte of the bytes copied.
 * The d values must be distinct, destination packets must not overlap each other, and the dense
 * and destination buffers must not overlap (none is checked; all hold for ebpf_verdict_queues'
 * and ebpf_gather's outputs). cap == 0, an empty queue and nothing to write are valid.
 * Returns, before any device call: EBPF_EINVAL for a NULL descriptor, index or count, queue >=
 * EBPF_NQUEUES, frames without src_frames, src_offsets or src_lens, frames with neither offsets
 * nor a non-zero stride, or a workspace that is too small; EBPF_ETOOBIG for n or cap > UINT32_MAX
 * or src_bytes > 4 GiB. */
int ebpf_scatter(const ebpf_scatter_desc* s, ebpf_stream_t stream);

/* The way out: one queue written as a classic libpcap byte stream -- the 24-byte global header,
 * then one record (16-byte record header + packet bytes) per packet of the queue, abutting. One
 * D2H copy of out[0, out_total[1]) is a capture file; out / out_offsets / out_lens with n =
 * out_total[0] is also an offsets + lens batch again (a capture in place, as ebpf_pcap_index
 * gives). All pointers are DEVICE pointers but file_header. */
#define EBPF_PCAP_SRC_RECORDS 1u /* the source batch is a capture in place: the 16 bytes before a
                                    packet are its record header, copied instead of synthesised */
#define EBPF_PCAP_SWAPPED     2u /* the record headers' fields are in the byte order opposite to
                                    the device's (a big-endian capture on this little-endian GPU) */
typedef struct ebpf_pcap_gather_desc {
  const uint8_t* frames;    /* the source batch, index, count and queue: exactly as in */
  const uint32_t* offsets;  /*   ebpf_gather_desc (packet i at frames + offsets[i], or frames + */
  const uint16_t* lens;     /*   i*stride when NULL; its length lens[i], or stride when NULL, then */
  uint64_t stride;          /*   stride <= 65535) */
  uint64_t n;               /* packets in the source batch (<= UINT32_MAX) */
  const uint32_t* index;    /* ebpf_verdict_queues' index, u32[n] */
  const uint32_t* count;    /* its count[EBPF_NQUEUES], READ ON THE DEVICE (no host sync) */
  uint32_t queue;           /* 0..EBPF_NQUEUES-1 */
  uint32_t flags;           /* EBPF_PCAP_* */
  uint8_t file_header[24];  /* HOST bytes, by value: the global header, written verbatim at output
                               byte 0 (the caller builds it, or copies the source capture's own) */
  uint32_t snaplen;         /* 0: no cut; else incl = min(len, snaplen) */
  const uint32_t* ts;       /* optional u32[n][2] (4-byte aligned), by SOURCE packet number: the
                               record's seconds and fraction (micro- or nanoseconds) */
  uint8_t* out;             /* u8[out_bytes] */
  uint64_t out_bytes;       /* <= 4 GiB (u32 offsets) */
  uint32_t* out_offsets;    /* optional u32[n]: record r's packet offset inside out */
  uint16_t* out_lens;       /* optional u16[n]: record r's incl */
  uint32_t* out_total;      /* u32[2], OVERWRITTEN: records written, the end byte */
  void* workspace;          /* optional scratch of ebpf_pcap_gather_workspace_bytes(n) bytes (8-byte
                               aligned, no zeroing); NULL => library-owned per (device, stream) */
  uint64_t workspace_bytes;
} ebpf_pcap_gather_desc;

uint64_t ebpf_pcap_gather_workspace_bytes(uint64_t n);

/* With m = count[queue] and s_j = index[start + j] the j-th packet number of that queue (start,
 * m clamped into index[0, n) as ebpf_scatter's): an entry with s_j >= n (none comes from
 * ebpf_verdict_queues) is NO RECORD -- nothing is written for it and no address is formed from it.
 * The others, in queue order, are the records r = 0, 1, ...; for record r of packet s:
 *   len = lens[s] or stride; incl = snaplen && snaplen < len ? snaplen : len;
 *   the record starts at byte 24 + the sum over earlier records of (16 + incl), its packet bytes
 *   16 bytes later (out_offsets[r]; out_lens[r] = incl); records abut, no padding anywhere;
 *   the packet bytes are the packet's first incl bytes as they are in `frames` when the call runs
 *   on the stream (after an EBPF_BATCH_WRITEBACK batch: the rewritten bytes);
 *   the 16 header bytes are four u32 {ts[s][0], ts[s][1], incl, len} -- {s, 0, incl, len} with ts
 *   == NULL: the source packet number as the timestamp -- each byte-swapped under
 *   EBPF_PCAP_SWAPPED. Under EBPF_PCAP_SRC_RECORDS a packet whose offset in frames (offsets[s] or
 *   s*stride) is >= 16 gets the 16 bytes before it instead, verbatim, but for the third field,
 *   which becomes incl (swapped under EBPF_PCAP_SWAPPED) when incl < len; the fourth (orig_len)
 *   is kept. A packet at an offset < 16 gets the synthesised header: nothing before `frames` is
 *   ever read.
 * Record r is written iff it ends at or below out_bytes (and 2^32 - 1); the ends ascend, so the
 * written records are a prefix, and out_total = {records written, end byte of the last one}, {0,
 * 24} with none. The global header is written iff out_bytes >= 24; otherwise out_total = {0, 0}.
 * Every byte of out at or past out_total[1] and every entry of out_offsets / out_lens at or past
 * out_total[0] is untouched (a record's last bytes are stored byte-exact: a neighbouring record is
 * never written twice and no wider word is read-modify-written). Source and output must not
 * overlap (not checked). Reads of frames stay inside the aligned 16-byte blocks that hold a byte
 * of a packet's first incl bytes, plus the 16 header bytes under EBPF_PCAP_SRC_RECORDS.
 * Asynchronous on `stream`, no host synchronisation (m is read on the device, the grid is sized
 * from n), two launches, no allocation when a workspace is passed. n == 0 is valid, launches
 * nothing and writes NOTHING (out_total included): there is no batch. Returns, before any device
 * call: EBPF_EINVAL for a NULL descriptor, index, count or out_total, a NULL frames with n > 0, a
 * NULL out with out_bytes > 0, no packet layout, stride > 65535 without lens, queue >=
 * EBPF_NQUEUES, a flag bit other than EBPF_PCAP_*, or a workspace that is too small or not 8-byte
 * aligned; EBPF_ETOOBIG for out_bytes > 4 GiB or n > UINT32_MAX. */
int ebpf_pcap_gather(const ebpf_pcap_gather_desc* p, ebpf_stream_t stream);

/* ---- RSS flow steering: which receive queue a packet arrives on ----
 * (new: no reference counterpart.) A NIC fills its RX queues by receive-side scaling: a Toeplitz
 * hash of the packet's address and port tuple (the Microsoft RSS specification), looked up in an
 * indirection table. ebpf_rss_hash is that hash for a whole batch, ebpf_steer the stable partition
 * of the packet numbers by the queue the table gives. Both are asynchronous and ordered on
 * `stream`, make no host synchronisation and allocate nothing when a workspace is passed. */
#define EBPF_RSS_IPV4      1u   /* src, dst                      (8 bytes)  */
#define EBPF_RSS_IPV4_TCP  2u   /* src, dst, sport, dport        (12 bytes) */
#define EBPF_RSS_IPV4_UDP  4u
#define EBPF_RSS_IPV6      8u   /* src, dst                      (32 bytes) */
#define EBPF_RSS_IPV6_TCP 16u   /* src, dst, sport, dport        (36 bytes) */
#define EBPF_RSS_IPV6_UDP 32u
typedef struct ebpf_rss_desc {
  const uint8_t* frames;    /* the batch, as in ebpf_gather_desc: packet i at frames + offsets[i], */
  const uint32_t* offsets;  /*   or frames + i*stride when NULL; its length lens[i], or stride */
  const uint16_t* lens;     /*   when NULL (then stride <= 65535). DEVICE pointers, any alignment */
  uint64_t stride;
  uint64_t n;               /* packets in the batch (<= UINT32_MAX) */
  uint8_t key[40];          /* HOST bytes, by value: the RSS key */
  uint32_t types;           /* the EBPF_RSS_* input types enabled */
  uint32_t* hash;           /* device u32[n] */
  uint8_t* type;            /* optional device u8[n]: the one EBPF_RSS_* bit used, 0 = not hashed */
} ebpf_rss_desc;

/* THE HASH (Toeplitz). The key is a big-endian bit string, key bit 0 the most significant bit of
 * key[0]. The input is a byte string taken in network order as it lies in the packet, input bit 0
 * the most significant bit of input byte 0. hash = the XOR, over every set input bit i, of the 32
 * key bits [i, i + 32) read as a big-endian number. A 36-byte input uses exactly the 40 key bytes.
 *
 * THE PARSE. Only the packet's bytes [0, len) are used. be16 = a big-endian 16-bit field.
 *   L2: the ethertype is be16 at 12; while it is 0x8100 or 0x88A8 (a VLAN tag, 4 bytes) the tag is
 *     skipped and the ethertype is the be16 4 bytes on, for up to two tags; the L3 header starts at
 *     o = 14 + 4 * tags. A third tag, or len < o, is NOT HASHED.
 *   IPv4 (ethertype 0x0800): needs len >= o + 20, a version nibble of 4 and IHL >= 5, else NOT
 *     HASHED. The L4 ports are used iff the packet is no fragment ((be16 at o + 6) & 0x3FFF == 0),
 *     the protocol at o + 9 is 6 (TCP) or 17 (UDP), the matching EBPF_RSS_IPV4_TCP / _UDP is
 *     enabled and len >= o + 4 * IHL + 4; the input is then src | dst | sport | dport (the bytes at
 *     o + 12 .. o + 20 and at o + 4 * IHL .. + 4) and the type that _TCP / _UDP bit. Otherwise,
 *     with EBPF_RSS_IPV4 enabled, the input is src | dst and the type EBPF_RSS_IPV4. Otherwise NOT
 *     HASHED.
 *   IPv6 (ethertype 0x86DD): needs len >= o + 40 and a version nibble of 6, else NOT HASHED. The
 *     ports (at o + 40) are used iff the next-header byte at o + 6 is itself 6 or 17, the matching
 *     EBPF_RSS_IPV6_TCP / _UDP is enabled and len >= o + 44: extension headers are not walked. The
 *     input is then src | dst | sport | dport (the bytes at o + 8 .. o + 40 and o + 40 .. o + 44).
 *     Otherwise, with EBPF_RSS_IPV6 enabled, the input is src | dst (type EBPF_RSS_IPV6).
 *     Otherwise NOT HASHED.
 *   Every other ethertype is NOT HASHED. NOT HASHED means hash[i] = 0 and type[i] = 0.
 * No byte at or past packet + len influences the result, and reads of `frames` stay inside the
 * aligned 16-byte blocks that hold a byte of the packet. Nothing is written but hash[0, n) and
 * type[0, n). n == 0 is valid and launches nothing. One launch, no scratch. Returns EBPF_EINVAL,
 * before any device call, for a NULL descriptor or hash, a NULL frames with n > 0, no packet layout
 * (no offsets, no lens, stride 0), stride > 65535 without lens, types == 0 or a types bit that is
 * no EBPF_RSS_*; EBPF_ETOOBIG for n > UINT32_MAX. */
int ebpf_rss_hash(const ebpf_rss_desc* r, ebpf_stream_t stream);

#define EBPF_STEER_MAX_QUEUES 64
#define EBPF_STEER_MAX_RETA   128

/* Device scratch ebpf_steer needs (8-byte aligned; needs no zeroing). */
uint64_t ebpf_steer_workspace_bytes(uint64_t n, uint32_t nq);

/* The stable partition of the packet numbers 0..n-1 into nq receive queues:
 *   queue(i) = reta[key[i] & (reta_len - 1)]
 * key: device u32[n] at any 4-byte aligned address (ebpf_rss_hash's hash, or any flow key). reta:
 * the indirection table, HOST u16[reta_len], copied by value; reta_len a power of two in
 * 1..EBPF_STEER_MAX_RETA, every entry < nq. reta == NULL selects Linux's default table (reta_len
 * is then ignored): 128 entries, reta[j] = j % nq. nq is 1..EBPF_STEER_MAX_QUEUES.
 * Once the call is complete on the stream: bounds[k] = {start_k, count_k} (device u32[nq][2]),
 * start_k = count_0 + ... + count_{k-1}; queue k is index[start_k .. start_k + count_k) (device
 * u32[n]); inside a queue the packet numbers ascend. The result is deterministic: a flow's packets
 * (one key) sit in one queue, in arrival order. Exactly n words of index and 2 * nq words of
 * bounds are written; with n == 0 bounds is all zero and index is untouched.
 *
 * THE PAIR LAYOUT IS A CONTRACT. ebpf_gather, ebpf_scatter and ebpf_pcap_gather read a queue as
 * start = count[0] + ... + count[queue - 1] and m = count[queue]. So
 *   count = bounds + 2 * k, queue = 1
 * hands steering queue k to those three calls as they stand (start = bounds[k][0], m =
 * bounds[k][1]); they read those two words of `count` and no other.
 *
 * workspace: device scratch of ebpf_steer_workspace_bytes(n, nq) bytes, one per stream; NULL =>
 * library-owned per (device, stream), in the buffer ebpf_verdict_queues' scratch lives in. Three
 * launches (count, bases, write) whose boundaries are the only ordering between workgroups.
 * Returns EBPF_EINVAL, before any device call, for nq outside 1..64, a reta_len that is no power of
 * two in 1..128, a table entry >= nq, a NULL bounds, a NULL key or index with n > 0, or a workspace
 * that is too small or not 8-byte aligned; EBPF_ETOOBIG for n > UINT32_MAX. */
int ebpf_steer(const uint32_t* key, uint64_t n, uint32_t nq, const uint16_t* reta,
               uint32_t reta_len, uint32_t* index, uint32_t* bounds, void* workspace,
               uint64_t workspace_bytes, ebpf_stream_t stream);

/* ---- Checksum offload: the Internet checksum of a whole batch ----
 * (new: no reference counterpart.) A NIC's RX descriptor says whether the IPv4 header checksum and
 * the TCP / UDP checksum of a packet were good, and its TX side writes them into packets that a
 * program rewrote. ebpf_csum_verify is the first for a whole batch, ebpf_csum_fill the second. Both
 * are asynchronous and ordered on `stream`, make no host synchronisation, need no scratch and
 * allocate nothing; each is one launch. */
#define EBPF_CSUM_IPV4_HDR 1u   /* the IPv4 header checksum */
#define EBPF_CSUM_TCP      2u   /* TCP over IPv4 and IPv6 */
#define EBPF_CSUM_UDP      4u   /* UDP over IPv4 and IPv6 */
/* status byte */
#define EBPF_CSUM_L3_GOOD  1u   /* fill: the header field was written */
#define EBPF_CSUM_L3_BAD   2u
#define EBPF_CSUM_L4_GOOD  4u   /* fill: the L4 field was written */
#define EBPF_CSUM_L4_BAD   8u
#define EBPF_CSUM_L4_NONE 16u   /* verify only: UDP over IPv4 whose checksum field is 0 (none sent) */
typedef struct ebpf_csum_desc {
  uint8_t* frames;          /* the batch, as in ebpf_rss_desc: packet i at frames + offsets[i], or */
  const uint32_t* offsets;  /*   frames + i*stride when NULL; its length lens[i], or stride when */
  const uint16_t* lens;     /*   NULL (then stride <= 65535). DEVICE pointers, any alignment. */
  uint64_t stride;          /*   ebpf_csum_verify only reads frames, ebpf_csum_fill WRITES it */
  uint64_t n;               /* packets in the batch (<= UINT32_MAX) */
  uint32_t what;            /* EBPF_CSUM_IPV4_HDR | _TCP | _UDP, non-zero */
  const uint8_t* verdict;   /* optional device u8[n]: selects packets by queue class */
  uint32_t queue_mask;      /* bit q set: packets of ebpf_verdict_queues' class q are processed (q =
                               v < 5 ? v : v == 0xFF ? 6 : 5); not applied when verdict == NULL */
  uint8_t* status;          /* optional device u8[n] (any alignment), OVERWRITTEN for all n */
} ebpf_csum_desc;

/* TERMS. be16 = a big-endian 16-bit field. fold(t): while (t >> 16) t = (t & 0xFFFF) + (t >> 16).
 * sum16(bytes) = the plain integer sum of the be16 words of a byte string, an odd last byte counting
 * as the high byte of a word whose low byte is 0. Only the packet's bytes [0, len) are used.
 *
 * SELECTION. With a verdict array, packet i is processed iff bit q(verdict[i]) of queue_mask is
 * set. A packet that is not selected gets status 0 and is not touched.
 *
 * THE PARSE.
 *   L2: exactly ebpf_rss_hash's: up to two VLAN tags are skipped, the L3 header starts at o = 14 +
 *     4 * tags; a third tag, len < o, or any ethertype but the two below gives status 0.
 *   IPv4 (ethertype 0x0800): needs len >= o + 20, a version nibble of 4, IHL >= 5 and len >= o + H,
 *     H = 4 * IHL; else status 0.
 *     L3 (with EBPF_CSUM_IPV4_HDR): GOOD iff fold(sum16(bytes [o, o + H))) == 0xFFFF, else BAD.
 *     L4: with T = be16 at o + 2 and p = o + H it needs ALL of: T >= H; o + T <= len (the packet
 *     holds the whole datagram; bytes past o + T are padding and ignored); no fragment ((be16 at
 *     o + 6) & 0x3FFF == 0); and, with L = T - H, either protocol (the byte at o + 9) 6 with
 *     EBPF_CSUM_TCP and L >= 20, or protocol 17 with EBPF_CSUM_UDP, L >= 8 and be16 at p + 4 == L.
 *     Otherwise no L4 bit is set. The sum is
 *       C = fold(sum16(src | dst) + protocol + L + sum16(bytes [p, p + L)))
 *     (src | dst the 8 bytes at o + 12), the checksum field at p + 16 for TCP and p + 6 for UDP.
 *   IPv6 (ethertype 0x86DD): needs len >= o + 40 and a version nibble of 6, else status 0. There is
 *     no L3 bit. L4 needs ALL of: the next-header byte at o + 6 is itself 6 or 17 and enabled
 *     (extension headers are not walked); with P = be16 at o + 4, p = o + 40 and L = P: p + L <=
 *     len; the same minimums on L and the same UDP length equality. The sum is
 *       C = fold(sum16(src | dst) + next header + L + sum16(bytes [p, p + L)))
 *     (src | dst the 32 bytes at o + 8).
 *
 * VERIFY. UDP over IPv4 whose two field bytes are 0 gets EBPF_CSUM_L4_NONE, and nothing is summed.
 * Otherwise EBPF_CSUM_L4_GOOD iff C == 0xFFFF, else EBPF_CSUM_L4_BAD. The definition is purely
 * arithmetic: a UDP over IPv6 field of 0 is summed like any other value. frames is only read.
 *
 * FILL. The field's two bytes count as 0 in the sum; the value is ~C & 0xFFFF, for UDP a value of
 * 0 becomes 0xFFFF; it is written big-endian at the field. The IPv4 header field at o + 10 is
 * filled by the same rule (over the header's sum), without the 0xFFFF substitution. status gets
 * EBPF_CSUM_L3_GOOD / _L4_GOOD for each field written, never _BAD or _NONE. Fill writes those
 * two-byte fields and NO other byte of frames: not the rest of the packet, not a neighbour that
 * abuts at any alignment, and no wider word is read-modify-written (the fields are stored byte by
 * byte).
 *
 * READS of frames stay inside the aligned 16-byte blocks that hold a byte of the packet, and no
 * byte at or past packet + len influences any result. Packets must not overlap (not checked).
 * Nothing else is written but status[0, n). n == 0 is valid and launches nothing.
 *
 * OUT OF SCOPE: ICMP and ICMPv6, IPv6 extension headers, SCTP, tunnelled inner headers, jumbograms
 * (an IPv6 payload length of 0 is taken as L = 0), partial (CHECKSUM_PARTIAL-style) sums.
 *
 * Both return EBPF_EINVAL, before any device call, for a NULL descriptor, a NULL frames with n > 0,
 * no packet layout (no offsets, no lens, stride 0), stride > 65535 without lens, what == 0 or a
 * what bit that is no EBPF_CSUM_*, a queue_mask bit at or above 1 << EBPF_NQUEUES (with or without
 * a verdict array); ebpf_csum_verify also for a NULL status. EBPF_ETOOBIG for n > UINT32_MAX. */
int ebpf_csum_verify(const ebpf_csum_desc* c, ebpf_stream_t stream);
int ebpf_csum_fill(const ebpf_csum_desc* c, ebpf_stream_t stream);

/* Human-readable message for an EBPF_E* code. */
const char* ebpf_strerror(int err);

/* Version string of the library (build configuration). */
/* Diagnostics: with EBPFEMU_TRACE=1 in the environment, the compiled fixed-slot kernel writes
 * per-wave s_memrealtime stamps (100 MHz) into a device buffer of `device`: a ring of 4 launches
 * of 65536 waves x 16 u64 (launch k in slot k % 4, zeroed once); wave w's 16 u64 at
 * w * 16 -- [0] entry, [1..10] after each tile, [12] before and [13] after the counter flush,
 * [14] XCC_ID << 32 | HW_ID, [15] tiles. NULL / 0 when off. */
int ebpf_debug_trace(int device, void** dev_ptr, size_t* bytes);

const char* ebpf_version(void);

#ifdef __cplusplus
}
#endif
#endif
