"""Child process of tests/test_opmatrix.py: the library reads EBPFEMU_FIXED_OCC once, when it
first compiles, so the fixed-slot kernel without its occupancy variant (ebpf_tile_jit_fixed) runs
in a fresh process with the switch the parent set. argv: <ebpf-emu_amd dir> <oracle dir> <tests
dir> <k>/<n>. Runs its share (every n-th, from the k-th) of the forward programs of the
operand-edge matrix (tests/opmatrix.py) over the 640-packet batch on fixed 64-byte slots on
cuda:0 -- full outputs and the production outputs -- checks each against the C oracle, prints one
JSON line and exits 0."""
import json
import sys


def main():
    sys.path[:0] = sys.argv[1:4]
    import torch

    import opmatrix as M
    import oracle
    from ebpf_emu import Program, _lib

    oracle.build()
    dev = torch.device("cuda", 0)
    prs = M.pairs()
    pkts, frames, kw = M.fixed_frames(prs, dev)
    out = {"programs": 0, "kernels": [], "failures": []}
    want = [_lib.EBPF_KERNEL_JIT_FIXED]
    route = "fixed slots, EBPFEMU_FIXED_OCC=0"
    k, n = (int(x) for x in sys.argv[4].split("/"))  # this process's share: every n-th program
    for p in [p for p in M.programs() if p.kind != "loop"][k::n]:
        img = p.image
        prog = Program(img)
        assert prog.compile(), p.name
        k = prog.batch_kernel(prog.make_batch(frames, max_steps=M.STEPS, **kw))
        if k not in out["kernels"]:
            out["kernels"].append(k)
        ref = M.oracle_ref(oracle, img, pkts)
        try:
            got = M.launch(prog, frames, kw, want)
            prod = M.launch(prog, frames, kw, want, prod=True)
            bad = (M.mismatch(p, route, img, prs, got, ref) or
                   M.mismatch(p, route + " (production outputs)", img, prs, prod, ref, full=got))
        except AssertionError as e:  # (the batch lands on another kernel)
            bad = f"{p.what} [{p.name}] route {route}: {e}"
        if bad and len(out["failures"]) < 5:
            out["failures"].append(bad)
        out["programs"] += 1
        prog.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
