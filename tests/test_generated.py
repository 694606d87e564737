"""The generated kernel text (csrc/gen_tile.py, run by the Makefile into build/gen/, never committed):
the generator is deterministic, writes exactly the files the sources include, and the sources
include nothing else that is not a hand-written file. Needs no built library."""
import filecmp
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ebpf-emu_amd", "csrc")
GENERATED = {"tile.inc", "tile_ids.h", "jit_tmpl.h", "tile_jit.inc", "tile_jit_loop.inc",
             "tile_jit_loop1.inc", "tile_jit_varl.inc"}
# written by the Makefile from the template kernels' assembly (csrc/embed.py), not by gen_tile.py
EMBEDDED = {"jit_template.h"}


def test_generator_is_deterministic_and_matches_the_includes(tmp_path):
    outs = [tmp_path / "a", tmp_path / "b"]
    for out in outs:
        out.mkdir()
        subprocess.run([sys.executable, os.path.join(CSRC, "gen_tile.py"), str(out)], check=True)
    assert set(os.listdir(outs[0])) == GENERATED and set(os.listdir(outs[1])) == GENERATED
    _, mismatch, errors = filecmp.cmpfiles(outs[0], outs[1], sorted(GENERATED), shallow=False)
    assert not mismatch and not errors, (mismatch, errors)

    included = set()
    for src in ("interp.hip", "jit.cpp", "host.cpp"):
        with open(os.path.join(CSRC, src)) as f:
            for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                if not os.path.isfile(os.path.join(CSRC, name)):  # (csrc/ or ../../include/)
                    assert name in GENERATED | EMBEDDED, f"{src} includes {name}"
                    included.add(name)
    assert included == GENERATED | EMBEDDED
