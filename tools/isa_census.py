"""Instruction census of one chain-kernel instantiation, per barrier-delimited step (CPU only, no GPU).

Compiles the translation unit that instantiates the kernel with build.py's flags to device assembly (or reads an
assembly file given with --asm), cuts the kernel's body at every `s_barrier` and prints, per step: MFMAs, VALU
instructions (and the most frequent VALU opcodes), moves, the longest run of consecutive moves, VALU in front of
the first MFMA (head) and behind the last one (tail), LDS and VMEM instructions and s_nop cycles; then the
kernel's register and spill counts.  Steps that carry the stochastic-rounding bf8 conversion are the backward
(input-gradient) steps of the 8-bit-stash kernels and are marked `bwd`.

    python tools/isa_census.py                       # the fused 8-bit-stash train kernel, width 256
    python tools/isa_census.py --kernel p2_128       # the backward half of the split phases, width 128
    python tools/isa_census.py --kernel 256,0,0,1,8,1,1,1,0,0 --all
"""
import argparse
import collections
import os
import re
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "nerf_for_angiography_amd", "csrc")

# template arguments of k_chain_bf16: F, X3, ENC, BWD, NW, SG, H16, S8, PHASE, ACTV
PARAMS = ("F", "X3", "ENC", "BWD", "NW", "SG", "H16", "S8", "PHASE", "ACTV")
INTS = {"F", "NW", "PHASE", "ACTV"}
PRESETS = {"s8_256": "256,0,0,1,8,1,1,1,0,0",      # bench.py's fused training step
           "p2_128": "128,0,0,1,8,1,1,1,2,0",      # backward half of the split phases (the reference's 4x128 model)
           "p2_256": "256,0,0,1,8,1,1,1,2,0"}
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed"]      # build.py's
SR_CVT = "v_cvt_scalef32_sr_bf8_f16"


def parse_kernel(spec: str) -> dict:
    vals = [int(v) for v in PRESETS.get(spec, spec).split(",")]
    if len(vals) != len(PARAMS):
        raise SystemExit(f"--kernel wants {len(PARAMS)} template arguments ({', '.join(PARAMS)}) or one of {sorted(PRESETS)}")
    return dict(zip(PARAMS, vals))


def mangled(k: dict) -> str:
    args = "".join(f"Li{k[p]}E" if p in INTS else f"Lb{1 if k[p] else 0}E" for p in PARAMS)
    return f"_Z12k_chain_bf16I{args}EvN3afx9ChainArgsE"


def unit_defines(k: dict) -> list:
    # afx_inst_chain16.hip: AFX_INST_BWD = 0 forward, 1 backward (PHASE 0), 2 split phases and activation variants
    bwd = 2 if (k["PHASE"] or k["ACTV"]) else (1 if k["BWD"] else 0)
    return [f"-DAFX_INST_F={k['F']}", f"-DAFX_INST_BWD={bwd}"]


def compile_asm(k: dict, out: str) -> None:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc] + FLAGS + unit_defines(k) + ["--cuda-device-only", "-S", os.path.join(CSRC, "afx_inst_chain16.hip"), "-o", out]
    subprocess.run(cmd, check=True)


def kernel_body(text: str, name: str) -> list:
    lines = text.splitlines()
    start = next((i for i, ln in enumerate(lines) if ln.split(";", 1)[0].strip() == f"{name}:"), None)
    if start is None:
        raise SystemExit(f"{name} is not in the assembly")
    body = []
    for ln in lines[start + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        s = ln.split(";", 1)[0].strip()
        if s and (not s.startswith(".") or s.endswith(":")):
            body.append(s)
    return body


def metadata(text: str, name: str) -> dict:
    """register counts from the kernel's code-object metadata"""
    out = {}
    m = re.search(rf"\.name:\s+{re.escape(name)}\s*\n", text)
    if not m:
        return out
    blk_start = text.rfind("\n  - ", 0, m.start())
    blk_end = text.find("\n  - ", m.end())
    blk = text[blk_start: blk_end if blk_end > 0 else len(text)]
    for key in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        r = re.search(rf"\.{key}:\s+(\d+)", blk)
        if r:
            out[key] = int(r.group(1))
    return out


def classify(op: str) -> str:
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_nop"):
        return "nop"
    return "other"


def steps(body: list) -> list:
    """the body cut at every s_barrier and behind every loop back-edge (a branch to an earlier label): per step the census counters"""
    labels = {ins[:-1]: i for i, ins in enumerate(body) if ins.endswith(":")}
    def fresh():
        return {"mfma": 0, "valu": 0, "mov": 0, "run": 0, "maxrun": 0, "head": 0, "tail": 0, "lds": 0, "vmem": 0,
                "nop": 0, "sr": 0, "loop": False, "ops": collections.Counter()}

    out, cur = [], fresh()
    for pos, ins in enumerate(body):
        if ins.endswith(":"):
            continue
        op = ins.split()[0]
        if op == "s_barrier":
            out.append(cur)
            cur = fresh()
            continue
        if op.startswith(("s_branch", "s_cbranch")) and labels.get(ins.split()[-1], pos) < pos:
            cur["loop"] = True
            out.append(cur)
            cur = fresh()
            continue
        op = re.sub(r"_(e32|e64|sdwa|dpp)$", "", op)
        c = classify(op)
        if c == "mfma":
            cur["mfma"] += 1
            cur["tail"] = 0
        elif c == "valu":
            cur["valu"] += 1
            cur["ops"][op] += 1
            if cur["mfma"] == 0:
                cur["head"] += 1
            cur["tail"] += 1
            if op == SR_CVT:
                cur["sr"] += 1
        elif c == "lds":
            cur["lds"] += 1
        elif c == "vmem":
            cur["vmem"] += 1
        elif c == "nop":
            r = re.match(r"s_nop\s+(\w+)", ins)
            cur["nop"] += (int(r.group(1), 0) if r else 0) + 1
        if op in ("v_mov_b32", "v_mov_b64"):
            cur["mov"] += 1
            cur["run"] += 1
            cur["maxrun"] = max(cur["maxrun"], cur["run"])
        elif c != "nop":
            cur["run"] = 0
    out.append(cur)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", default="s8_256", help=f"preset ({', '.join(sorted(PRESETS))}) or the ten template arguments")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep", help="write the compiled assembly here")
    ap.add_argument("--all", action="store_true", help="print every step, not only the MFMA-carrying ones")
    ap.add_argument("--top", type=int, default=6, help="VALU opcodes listed per step")
    args = ap.parse_args()
    k = parse_kernel(args.kernel)
    name = mangled(k)
    if args.asm:
        with open(args.asm) as f:
            text = f.read()
    else:
        with tempfile.TemporaryDirectory() as td:
            out = args.keep or os.path.join(td, "unit.s")
            compile_asm(k, out)
            with open(out) as f:
                text = f.read()
    body = kernel_body(text, name)
    st = steps(body)
    md = metadata(text, name)
    print(f"k_chain_bf16<{', '.join(str(k[p]) for p in PARAMS)}>: {sum(not i.endswith(':') for i in body)} instructions, {len(st)} barrier-delimited steps")
    print()
    print("| step | kind | MFMA | VALU | head | tail | v_mov | longest v_mov run | LDS | VMEM | s_nop cycles | top VALU |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for i, s in enumerate(st):
        if not args.all and s["mfma"] == 0:
            continue
        top = ", ".join(f"{o} {n}" for o, n in s["ops"].most_common(args.top))
        print(f"| {i} | {'bwd' if s['sr'] else ''}{' (loop end)' if s['loop'] else ''} | {s['mfma']} | {s['valu']} | {s['head']} | {s['tail']} | {s['mov']} | {s['maxrun']} "
              f"| {s['lds']} | {s['vmem']} | {s['nop']} | {top} |")
    print()
    bwd = [s for s in st if s["sr"] and s["mfma"]]
    if bwd:
        v = [s["valu"] for s in bwd]
        print(f"backward steps: {len(bwd)}; VALU per step min {min(v)}, max {max(v)} (max/min {max(v) / max(1, min(v)):.2f}); "
              f"longest v_mov run {max(s['maxrun'] for s in bwd)}")
    tot = collections.Counter()
    for s in st:
        for key in ("mfma", "valu", "mov", "lds", "vmem", "nop"):
            tot[key] += s[key]
    print(f"whole kernel: MFMA {tot['mfma']}, VALU {tot['valu']}, v_mov {tot['mov']}, LDS {tot['lds']}, VMEM {tot['vmem']}, s_nop cycles {tot['nop']}")
    print("registers: " + ", ".join(f"{key} {val}" for key, val in md.items()))


if __name__ == "__main__":
    main()
