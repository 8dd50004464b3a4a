"""Compile-only checks of the backward chain's instruction schedule (no GPU): the 256-wide 8-bit-stash train kernel
does not spill, carries one tile epilogue per backward step (no step with the sunk epilogues of several tiles) and
has no register-copy block between layers.  tools/isa_census.py does the counting."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _census():
    spec = importlib.util.spec_from_file_location("isa_census", os.path.join(ROOT, "tools", "isa_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_backward_steps_of_the_256_wide_s8_kernel_carry_one_epilogue_each(tmp_path):
    c = _census()
    k = c.parse_kernel("s8_256")
    out = str(tmp_path / "unit.s")
    c.compile_asm(k, out)
    with open(out) as f:
        text = f.read()
    name = c.mangled(k)
    md = c.metadata(text, name)
    assert md.get("vgpr_spill_count") == 0, md
    bwd = [s for s in c.steps(c.kernel_body(text, name)) if s["sr"] and s["mfma"]]
    assert len(bwd) >= 8, len(bwd)      # the two-layer body of the chain loop: 2 x 4 steps
    # the first step also seeds the chain and the last one runs on into the code behind the loop: the steps between are the loop body
    valu = [s["valu"] for s in bwd[1:-1]]
    assert max(valu) <= 1.5 * min(valu), valu
    assert max(s["maxrun"] for s in bwd) < 32, [s["maxrun"] for s in bwd]
