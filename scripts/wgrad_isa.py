"""Instruction census of the MFMA loops of k_wgrad / k_wgrad_wide in the gfx950 device assembly.

    python scripts/wgrad_isa.py [ndp.s]

Without an argument the assembly is produced with the command line of scripts/isa.sh (hipcc on PATH or in
/opt/rocm/bin) into a temporary directory.  For each kernel it prints the register budget and, for every innermost
loop that holds MFMAs, what one pass through the loop executes: MFMAs, vector loads, every s_waitcnt vmcnt(N),
accumulator moves, v_mov_b64, conditional branches, conversions, s_nop.  tests/test_wgrad_isa.py asserts on the same
census.  Everything here reads the text the installed compiler emits: a different compiler may lay the loops out
differently without being wrong.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndivplanning_amd", "csrc")
KERNELS = ("k_wgrad", "k_wgrad_wide")

_BLOCK = re.compile(r"^(?:(\.LBB\d+_\d+):|; %bb\.\d+:)")
_INLOOP = re.compile(r"in Loop: Header=(BB\d+_\d+)")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return exe if os.path.exists(exe) else None


def compile_asm(out_dir, extra_flags=()):
    """Device assembly of ndp_kernels.hip (scripts/isa.sh's command line) -> path of the .s file."""
    out = os.path.join(str(out_dir), "ndp.s")
    cmd = [hipcc(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
           "-Wno-pass-failed", "-Wno-invalid-offsetof"] + list(extra_flags) + [os.path.join(CSRC, "ndp_kernels.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return out


def kernel_text(lines, name):
    """(body lines, metadata dict) of the kernel whose mangled symbol holds `<len><name>E` (ndp::name)."""
    tag = "%d%sE" % (len(name), name)
    start = next(i for i, l in enumerate(lines) if re.match(r"^_ZN3ndp%s\w*:" % tag, l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    meta = {}
    for l in lines[start:end + 40]:                    # the .amdhsa_ block precedes .Lfunc_end, the summary comments follow it
        m = re.match(r"^\s+\.amdhsa_(next_free_vgpr|accum_offset|private_segment_fixed_size)\s+(\d+)", l)
        if m:
            meta[m.group(1)] = int(m.group(2))
        m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy): (\d+)", l)
        if m:
            meta[m.group(1)] = int(m.group(2))
            if m.group(1) == "Occupancy":
                break
    return lines[start:end], meta


def innermost_loops(body):
    """[[line, ...]] the lines of every innermost loop, by the loop annotations the compiler writes on each block's first
    line ('=>This Inner Loop Header', 'in Loop: Header=BBn_m').  A backward branch alone does not make a loop: block
    placement produces those too."""
    loops, member = {}, None
    for l in body:
        m = _BLOCK.match(l)
        if m:
            member = None
            if "This Inner Loop Header" in l:
                member = m.group(1).lstrip(".L")
                loops[member] = []
            else:
                h = _INLOOP.search(l)
                if h and h.group(1) in loops:
                    member = h.group(1)
        if member is not None:
            loops[member].append(l)
    return list(loops.values())


def census(lines):
    ins = [l.split(";")[0].strip() for l in lines]
    ins = [l for l in ins if l and not l.endswith(":") and not l.startswith(".")]
    ops = [l.split()[0] for l in ins]
    waits = [int(m.group(1)) for l in ins if l.startswith("s_waitcnt") for m in [_VMCNT.search(l)] if m]
    cond = [l for l in ins if l.startswith("s_cbranch")]
    return {
        "instructions": len(ins),
        "mfma": sum(o.startswith("v_mfma") for o in ops),
        "vmem_loads": sum(o.startswith(("global_load", "buffer_load", "flat_load")) for o in ops),
        "lds": sum(o.startswith("ds_") or "_lds_" in o for o in ops),
        "vmcnt": waits,
        "vmcnt0": sum(w == 0 for w in waits),
        "accvgpr_read": sum(o.startswith("v_accvgpr_read") for o in ops),
        "accvgpr_write": sum(o.startswith("v_accvgpr_write") for o in ops),
        "v_mov_b64": sum(o.startswith("v_mov_b64") for o in ops),
        "cond_branches": len(cond),
        "branches_inside": len(cond) - 1,          # all but the back-edge
        "v_cvt": sum(o.startswith("v_cvt") for o in ops),
        "s_nop": sum(o == "s_nop" for o in ops),
        "v_mul_64": sum(o.startswith(("v_mad_u64", "v_mad_i64", "v_mul_hi")) for o in ops),
    }


def wgrad_loops(path):
    """{kernel: (meta, [census of each innermost MFMA loop that is wgrad_block's])}.  wgrad_wide's own loop is the one
    that reads its operands from LDS; wgrad_block's loops touch no LDS."""
    with open(path) as f:
        lines = f.read().splitlines()
    out = {}
    for k in KERNELS:
        body, meta = kernel_text(lines, k)
        cs = [census(ls) for ls in innermost_loops(body)]
        out[k] = (meta, [c for c in cs if c["mfma"] > 0 and c["lds"] == 0])
    return out


def main(argv):
    if len(argv) > 1:
        res = wgrad_loops(argv[1])
    else:
        if hipcc() is None:
            sys.exit("hipcc not found")
        with tempfile.TemporaryDirectory() as d:
            res = wgrad_loops(compile_asm(d))
    for k, (meta, loops) in res.items():
        print("%s: VGPRs %s, AGPRs %s, scratch %s, occupancy %s" % (
            k, meta.get("NumVgprs"), meta.get("NumAgprs"), meta.get("ScratchSize"), meta.get("Occupancy")))
        for c in loops:
            print("  loop: %(mfma)d MFMA, %(instructions)d instructions, %(vmem_loads)d loads, vmcnt %(vmcnt)s, "
                  "accvgpr r/w %(accvgpr_read)d/%(accvgpr_write)d, v_mov_b64 %(v_mov_b64)d, branches inside %(branches_inside)d, "
                  "v_cvt %(v_cvt)d, s_nop %(s_nop)d, 64-bit mul %(v_mul_64)d" % c)


if __name__ == "__main__":
    main(sys.argv)
