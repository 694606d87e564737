"""Child process of tests/test_loadmatrix.py: the library reads EBPFEMU_FIXED_OCC once, when it
first compiles, so the fixed-slot kernel without its occupancy variant (ebpf_tile_jit_fixed) runs
in a fresh process with the switch the parent set. argv: <ebpf-emu_amd dir> <oracle dir> <tests
dir> <k>/<n>. Runs its share (every n-th, from the k-th) of the forward programs of the load-edge
matrix (tests/loadmatrix.py) over their batches on fixed 64-byte slots on cuda:0 -- full outputs
and the production outputs -- checks each against the C oracle, prints one JSON line and exits
0."""
import json
import sys


def main():
    sys.path[:0] = sys.argv[1:4]
    import torch

    import loadmatrix as M
    import oracle
    import test_loadmatrix as T
    from ebpf_emu import Program, _lib

    oracle.build()
    dev = torch.device("cuda", 0)
    out = {"programs": 0, "kernels": [], "failures": []}
    route = "fixed slots, stride 64, EBPFEMU_FIXED_OCC=0"
    k, n = (int(x) for x in sys.argv[4].split("/"))  # this process's share: every n-th program
    for p in [p for p in M.programs() if p.kind != "loop"][k::n]:
        prog = Program(p.image())
        assert prog.compile(), p.name
        bad = T.run_route(prog, p, route, "plain", T._staged(p.batch, "plain", ("fixed", 64), dev),
                          {}, None, [_lib.EBPF_KERNEL_JIT_FIXED], oracle)
        if bad and len(out["failures"]) < 5:
            out["failures"].append(bad)
        out["programs"] += 1
        prog.close()
        T._REF.clear()
    out["kernels"] = sorted(T.REACHED)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
