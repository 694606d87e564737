"""The route table: where ebpf_run_batch sends a batch, asked of the three route queries.

A deterministic table of rows (program, batch description, outputs requested). For each row the
answers of Program.batch_kernel, batch_staged and workspace_bytes are compared by
tests/test_routes.py with tests/golden/routes.json, which holds the answers of the commit before
the batch plan (host.cpp plan_batch) existed: the plan must route every batch as the scattered
decision it replaced did.

    python tests/routes.py --record [--out PATH]

writes the fixture from the library next to this checkout (it needs the GPU: a query uploads the
program). To re-record against another commit, copy this module into a checkout of that commit,
build it there and run it there. The queries read no packet memory: a row's frames, offsets and
lens are addresses inside one small device buffer, chosen for their alignment only, and no kernel
is launched.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "routes.json")

# a tier-1 program whose store leaves the stack window (r10 - 128: past kStackMax)
T1_SRC = "mov r3, r10\nadd r3, -128\nstxdw [r3+0], r2\nldxdw r0, [r3+0]\nexit"

# (frames offset, stride, offsets at, lens at): byte offsets into the device buffer, None = absent
LAYOUTS = {
    "s64": (0, 64, None, None),
    "s64+8": (8, 64, None, None),
    "s1504": (0, 1504, None, None),
    "s60": (0, 60, None, None),
    "ol": (0, 0, 64, 128),
    "o2l": (0, 0, 66, 128),
    "ol2": (0, 0, 64, 130),
    "l": (0, 64, None, 128),
}
NS = (64, 16383, 16384)  # 16384: the binning threshold


def programs():
    """name -> program image: one of each shape the router tells apart."""
    from ebpf_emu import workloads as W
    from ebpf_emu.asm import assemble

    names = ["5tuple", "5tuple_xdp", "nat", "mac_swap_tx", "responder", "acl", "acl_rules",
             "checksum", "checksum_xdp_reload", "checksum_stack", "5tuple_call"]
    progs = {k: W.program(k) for k in names}
    progs["t1_store"] = assemble(T1_SRC)
    # a forward program of 63..256 micro-ops other than the ACL (no_jit: dag_kernel)
    progs["rules12"] = assemble(W.acl_rules_source(rules=12))
    return progs


def table():
    """[(row name, program name, batch kwargs)]: layout x n for every program, then one axis at a
    time around the base row (s64, n = 64, mem_size 1024, r10 512, no flags, verdict only)."""
    rows = []
    for prog in programs():
        def row(tag, **kw):
            rows.append((f"{prog} {tag}", prog, kw))

        for lay in LAYOUTS:
            for n in NS:
                row(f"{lay} {n}", layout=lay, n=n)
            row(f"{lay} xdp", layout=lay, xdp_md=True)
        for flag in ("generic", "no_jit", "writeback"):
            row(flag, **{flag: True})
        row("xdp+wb", xdp_md=True, writeback=True)
        row("ol 16384 no_jit", layout="ol", n=16384, no_jit=True)
        row("ol 16384 xdp", layout="ol", n=16384, xdp_md=True)
        row("ol wb", layout="ol", writeback=True)
        for o in ("mem", "regs", "fp"):
            row(f"out {o}", outs=(o,))
        row("xdp out mem", xdp_md=True, outs=("mem",))
        row("init_regs", init_regs=True)
        row("xdp init_regs", xdp_md=True, init_regs=True)
        row("init_fp", init_fp=True)
        row("steps 8", max_steps=8)
        for m in (64, 4096):
            row(f"mem {m}", mem_size=m)
        for r10 in (32, 136, 510):  # 32: the stack window inside the 64-byte slot
            row(f"r10 {r10}", r10=r10)
    rows.append(("5tuple steps 0", "5tuple", dict(max_steps=0)))  # rejected: EBPF_EINVAL
    rows.append(("5tuple xdp mem 65536", "5tuple", dict(xdp_md=True, mem_size=65536)))  # likewise
    return rows


class Asker:
    """Answers rows on one device: the programs loaded once, one device buffer for the addresses."""

    def __init__(self, device=0):
        import torch

        from ebpf_emu import Program

        self.device = device
        self.buf = torch.zeros(4096, dtype=torch.uint8, device=torch.device("cuda", device))
        self.progs = {k: Program(img) for k, img in programs().items()}
        self.cus = torch.cuda.get_device_properties(device).multi_processor_count

    def batch(self, prog, layout="s64", n=64, outs=(), init_regs=False, init_fp=False, **kw):
        from ebpf_emu import _lib

        base = self.buf.data_ptr()
        assert base % 256 == 0
        f, stride, o, ln = LAYOUTS[layout]
        b = self.progs[prog].make_batch(self.buf, n=n, stride=stride, **kw)
        b.frames = base + f
        b.offsets = base + o if o is not None else None
        b.lens = base + ln if ln is not None else None
        if init_regs:
            b.init_regs = base + 1024
        if init_fp:
            b.init_fp = base + 2048
            b.init_fp_len = 1
        out = _lib.BatchOut()
        out.verdict = base + 3072
        for name in outs:
            setattr(out, name, base + 3072)
            if name == "fp":
                out.fp_len = base + 3072
        return b, out

    def ask(self, prog, kw):
        """[kernel id or EBPF_E*, staged 0 / 1 or EBPF_E*, workspace bytes]"""
        from ebpf_emu import _lib

        b, out = self.batch(prog, **kw)
        p = self.progs[prog]
        ans = []
        for q in (p.batch_kernel, p.batch_staged):
            try:
                ans.append(int(q(b, out, self.device)))
            except _lib.EbpfError as e:
                ans.append(e.code)
        ans.append(p.workspace_bytes(b, self.device))
        return ans


def coverage(asker, answers):
    """What the recorded table must show, so that a table which misses a route cannot be
    committed: every kernel id, both values of staged, a deopt launch with its pass, one without,
    and a binned batch. (The last three are not among the answers: they follow from the kernel id
    and the program's properties by the rules of DESIGN.md 3.6.)"""
    from ebpf_emu import _lib as L

    missing = []
    ids = {a[0] for a in answers.values()}
    missing += [f"kernel id {i}" for i in range(len(L.KERNEL_NAMES)) if i not in ids]
    missing += [f"staged {s}" for s in (0, 1) if s not in {a[1] for a in answers.values()}]
    seen = set()
    for name, prog, kw in table():
        kid = answers[name][0]
        p = asker.progs[prog]
        plain = not kw.get("init_regs") and kw.get("r10", 512) == 512 and \
            kw.get("mem_size", 1024) == 1024
        if p.store_mode and kid in (L.EBPF_KERNEL_JIT_STACK, L.EBPF_KERNEL_JIT_VARL_STACK) and \
                p.store_mode_no_deopt and plain:
            seen.add("deopt launch, no pass")
        if (p.store_mode and kid == L.EBPF_KERNEL_JIT_VAR_STACK) or \
                (p.promoted and kid == L.EBPF_KERNEL_JIT_LOOP):
            seen.add("deopt launch with its pass")
        if kw.get("layout") == "ol" and kw.get("n", 64) >= 16384 and not kw.get("xdp_md") and \
                (kid == L.EBPF_KERNEL_TILE_LOOP or
                 (kid == L.EBPF_KERNEL_JIT_LOOP and not p.promoted and
                  p.jit_loop_kernel() == "ebpf_tile_jit_loop")):
            seen.add("binned")
    missing += sorted({"deopt launch, no pass", "deopt launch with its pass", "binned"} - seen)
    return missing


def record(path):
    asker = Asker()
    answers = {name: asker.ask(prog, kw) for name, prog, kw in table()}
    assert len(answers) == len(table()), "row names repeat"
    lines = ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}"
                       for k, v in answers.items())
    with open(path, "w") as f:
        f.write('{"cus": %d, "rows": {\n%s\n}}\n' % (asker.cus, lines))
    print(f"{len(answers)} rows -> {path}")
    missing = coverage(asker, answers)
    if missing:
        os.replace(path, path + ".incomplete")
        sys.exit("the table misses: " + ", ".join(missing))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ebpf-emu_amd"))
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--out", default=FIXTURE)
    record(ap.parse_args().out)
