"""Instruction census of the MFMA loops of a HIP source file (gfx950), from hipcc's own assembly.

    python3 tools/isa_census.py resunet_a_mltsk_keras_amd/csrc/conv_strip.hip [name-filter] [-D...] [--ops]
    python3 tools/isa_census.py NEW.hip [name-filter] [-I...] --against OLD.hip

For every kernel whose (demangled) name contains the filter, every innermost-first loop (a label .. the last
backward branch to it) that holds MFMAs is listed with the STATIC count of its instructions by issue class:
MFMA, VALU (everything else v_*), SALU (s_* without waits / nops / barriers / branches), LDS (ds_*), VMEM
(buffer_* / global_*), wait (s_waitcnt, s_nop, s_barrier), branch.  Static = every path of the loop body once;
bodies here are straight-line apart from uniform skips.  --ops adds the histogram of VALU mnemonics.

--against OTHER.hip compiles both files and says, kernel by kernel, whether the instruction streams are the same (comments and
directives stripped, block labels numbered in order of appearance), with the instruction count and the metadata's .vgpr_count,
.sgpr_count, .group_segment_fixed_size (LDS) and .private_segment_fixed_size (scratch) of either file: what a refactor that
means to leave a kernel alone has to show.
"""
import collections
import re
import subprocess
import sys
import tempfile
import os

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def asm_of(src, defs):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src, "-o", out] + defs
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        text = f.read()
    os.unlink(out)
    return text


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, p.stdout.splitlines()))


def classify(m):
    if m.startswith("v_mfma") or m.startswith("v_smfma"):
        return "MFMA"
    if m.startswith("v_"):
        return "VALU"
    if m.startswith("ds_"):
        return "LDS"
    if m.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    if m.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep", "s_setprio")):
        return "wait"
    if m.startswith(("s_cbranch", "s_branch", "s_endpgm")):
        return "branch"
    if m.startswith("s_"):
        return "SALU"
    return "other"


def functions(text):
    cur, body = None, []
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            yield cur, body
            cur = None
            continue
        body.append(line)


def census(body):
    # instruction list with label positions
    ins, labels = [], {}
    for line in body:
        s = line.strip()
        if not s or s.startswith((";", ".")) and not re.match(r"^\.LBB\w+:", s):
            if re.match(r"^\.LBB\w+:", s):
                pass
            else:
                continue
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        tok = s.split()
        if not tok or tok[0].startswith((";", ".")):
            continue
        ins.append((tok[0], s))
    loops = {}
    for i, (m, s) in enumerate(ins):
        if m.startswith(("s_cbranch", "s_branch")):
            tgt = s.split()[-1]
            if tgt in labels and labels[tgt] <= i:
                loops[tgt] = max(loops.get(tgt, -1), i)
    out = []
    for tgt, end in sorted(loops.items(), key=lambda kv: kv[1] - labels[kv[0]]):
        seg = ins[labels[tgt]:end + 1]
        c = collections.Counter(classify(m) for m, _ in seg)
        if c["MFMA"] == 0:
            continue
        ops = collections.Counter(m for m, _ in seg if classify(m) == "VALU")
        out.append((tgt, len(seg), c, ops))
    return out


def stream(body):
    """The instructions of a function body: no comments, no directives, block labels renamed by first appearance."""
    names, out = {}, []
    for line in body:
        s = line.split(";")[0].strip()
        if not s or (s.startswith(".") and not re.match(r"^\.LBB\w+:", s)):
            continue
        out.append(re.sub(r"\.LBB\w+", lambda m: names.setdefault(m.group(0), "L%d" % len(names)), " ".join(s.split())))
    return out


META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def metadata(text):
    """{mangled kernel name: {key: int}} from the kernel entries of the amdhsa metadata."""
    out, cur = {}, {}
    for line in text.splitlines() + ["  - ."]:
        if line.startswith("  - ."):
            if ".name" in cur:
                out[cur[".name"]] = cur
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"^    (\.\w+):\s+(\S+)\s*$", line)
        if m:
            cur[m.group(1)] = m.group(2)
    return out


def against(src, other, filt, defs):
    sides = []
    for f in (other, src):
        text = asm_of(f, defs)
        funcs = dict(functions(text))
        names = demangle(list(funcs))
        meta = metadata(text)
        sides.append({names[f].replace("(anonymous namespace)::", "").split("(")[0]: (stream(b), meta.get(f, {})) for f, b in funcs.items() if f in meta})
    old, new = sides
    print("%-52s %-9s %13s %9s %9s %13s %9s" % ("kernel (old / new)", "identical", "instructions", "VGPR", "SGPR", "LDS", "scratch"))
    for name in sorted(set(old) | set(new)):
        if filt and filt not in name:
            continue
        (so, mo), (sn, mn) = old.get(name, ([], {})), new.get(name, ([], {}))
        cols = ["%s / %s" % (mo.get("." + k, "-"), mn.get("." + k, "-")) for k in META]
        print("%-52s %-9s %13s %9s %9s %13s %9s" % (name, "yes" if so == sn else "no",
                                                   "%d / %d" % tuple(sum(not i.endswith(":") for i in x) for x in (so, sn)), *cols))


def main():
    argv = sys.argv[1:]
    other = None
    if "--against" in argv:
        i = argv.index("--against")
        other = argv[i + 1]
        del argv[i:i + 2]
    args = [a for a in argv if not a.startswith("-")]
    defs = [a for a in argv if a.startswith("-") and a != "--ops"]
    if other:
        return against(args[0], other, args[1] if len(args) > 1 else "", defs)
    show_ops = "--ops" in sys.argv
    src = args[0]
    filt = args[1] if len(args) > 1 else ""
    text = asm_of(src, defs)
    funcs = list(functions(text))
    names = demangle([f for f, _ in funcs])
    for f, body in funcs:
        name = names.get(f, f)
        if filt and filt not in name:
            continue
        res = census(body)
        if not res:
            continue
        print(name.split("(")[0])
        for tgt, n, c, ops in res:
            print("  loop %-12s %5d instr  MFMA %3d  VALU %4d  SALU %4d  LDS %3d  VMEM %3d  wait %3d  branch %2d   VALU/MFMA %.1f" % (
                tgt, n, c["MFMA"], c["VALU"], c["SALU"], c["LDS"], c["VMEM"], c["wait"], c["branch"], c["VALU"] / c["MFMA"]))
            if show_ops:
                print("     " + "  ".join("%s %d" % kv for kv in ops.most_common(24)))


if __name__ == "__main__":
    main()
