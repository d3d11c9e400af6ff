#!/usr/bin/env python3
"""Static counts of the FFT kernels' generated code, from the device assembly the build keeps (csrc/build/smst_fft-hip-amdgcn-amd-amdhsa-gfx950.s):
per instantiation the registers, scratch and occupancy the compiler reports, and for its frame loop (hop loop in kSynthEmitTeams) the
instructions by class.  Nothing is run.

The frame loop of a function is taken from the text: a loop is a backward branch to a label of the same function, its body the instructions
between the two; the frame loop is the innermost such body that holds the transform (nine tenths of the function's packed-f32 instructions: the barrier spins
and the edge loops hold none, a branch back inside the transform holds a part of it, the item loop around kSynthEmitTeams' hop loop contains it).  The kernels of one frame per workgroup (kAnalyseFast -- two
copies of the transform, the usual case and the general one --, kSynthFast, kAnalyse, kSynth) are counted whole.

kAnalyseTeamPairs' loop holds two copies of the transform: the pass of two frames in lockstep (two thirds of its packed instructions) and the
pass with one wanted frame.

usage: fft_core_isa_table.py [<label>=]<assembly> [[<label>=]<assembly of another build> ...]   -> one table per file on stdout
       fft_core_isa_table.py --check-budgets <assembly>   -> exit status 1 unless the build keeps kAnalyseTeamPairs' budgets (csrc/Makefile runs this):
       its eight instantiations exist, none uses scratch, each is compiled for exactly two waves per SIMD"""
import re
import subprocess
import sys

KERNELS = ("kAnalyseTeamPairs", "kAnalyseTeams", "kSynthTeams", "kSynthEmitTeams", "kAnalyseFast", "kSynthFast", "kAnalyse", "kSynth")
PACKED = re.compile(r"v_pk_(mul|fma|add)_f32")
SCALAR_F32 = re.compile(r"v_(mul|fma|fmac|add|sub|subrev|mac|mad)_f32")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def functions(text):
    """-> [(mangled name, [lines of the body], {metadata})]"""
    out, cur, where = [], None, None
    for line in text.split("\n"):
        start = re.match(r"^(_ZN4smst\w+):", line)
        if start:
            cur, where = (start.group(1), [], {}), "body"
            out.append(cur)
        elif cur and where == "body" and re.match(r"^\.Lfunc_end\d+:", line):
            where = "meta"
        elif cur and where == "body":
            cur[1].append(line)
        elif cur and where == "meta":
            k = re.match(r"^; (TotalNumVgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", line)
            if k:
                cur[2][k.group(1)] = int(k.group(2))
    return out


def instructions(lines):
    """-> [(index of the line, mnemonic)], {label: position among the instructions}"""
    ins, labels = [], {}
    for i, line in enumerate(lines):
        s = line.split(";")[0].strip()
        if not s or s.startswith("."):
            lab = re.match(r"^(\.LBB\d+_\d+):", s)
            if lab:
                labels[lab.group(1)] = len(ins)
            continue
        ins.append((i, s.split()[0], s))
    return ins, labels


def frame_loop(ins, labels):
    spans = []
    for pos, (_, op, s) in enumerate(ins):
        if op.startswith("s_cbranch") or op == "s_branch":
            target = s.split()[-1]
            if target in labels and labels[target] <= pos:
                spans.append((labels[target], pos))
    packed = [1 if PACKED.match(op) else 0 for _, op, _ in ins]
    big = [sp for sp in spans if sum(packed[sp[0]:sp[1] + 1]) >= 0.9*sum(packed)]
    inner = [sp for sp in big if not any(o != sp and sp[0] <= o[0] and o[1] <= sp[1] for o in big)]
    return min(inner, key=lambda sp: sp[1] - sp[0]) if inner else None


def classify(ops):
    c = dict(instructions=len(ops), valu=0, packed=0, scalar_f32=0, mov32=0, mov64=0, xor=0)
    for op in ops:
        if op.startswith("v_"):
            c["valu"] += 1
        if PACKED.match(op):
            c["packed"] += 1
        elif SCALAR_F32.match(op):
            c["scalar_f32"] += 1
        elif op.startswith("v_mov_b32"):
            c["mov32"] += 1
        elif op.startswith("v_mov_b64") or op.startswith("v_pk_mov_b32"):
            c["mov64"] += 1
        elif op.startswith("v_xor_b32"):
            c["xor"] += 1
    return c


def table(arg):
    label, _, path = arg.rpartition("=")
    text = open(path).read()
    funcs = [f for f in functions(text)]
    names = demangle([f[0] for f in funcs])
    rows = []
    for mangled, lines, meta in funcs:
        name = names[mangled]
        short = re.sub(r"^void smst::", "", name).split("(")[0]
        if not short.startswith(KERNELS):
            continue
        ins, labels = instructions(lines)
        span = frame_loop(ins, labels) if "Team" in short else None
        ops = [op for _, op, _ in (ins[span[0]:span[1] + 1] if span else ins)]
        rows.append((short, "loop" if span else "whole", meta, classify(ops)))
    rows.sort()
    print("# %s" % (label or path))
    print("%-58s %-5s %5s %5s %7s %4s %6s | %6s %5s %6s %10s %9s %9s %9s" % ("kernel", "body", "VGPR", "SGPR", "scratch", "occ", "LDS", "instr", "VALU", "packed", "scalar f32", "v_mov_b32", "v_mov_b64", "v_xor_b32"))
    for short, body, meta, c in rows:
        print("%-58s %-5s %5d %5d %7d %4d %6d | %6d %5d %6d %10d %9d %9d %9d" % (short, body, meta["TotalNumVgprs"], meta["TotalNumSgprs"], meta["ScratchSize"], meta["Occupancy"],
              meta["LDSByteSize"], c["instructions"], c["valu"], c["packed"], c["scalar_f32"], c["mov32"], c["mov64"], c["xor"]))
    print()


def check_budgets(path):
    funcs = functions(open(path).read())
    names = demangle([f[0] for f in funcs])
    pairs = [(names[m], meta) for m, _, meta in funcs if "kAnalyseTeamPairs<" in names[m]]
    bad = ["%s: %s" % (n, meta) for n, meta in pairs if meta.get("ScratchSize") != 0 or meta.get("Occupancy") != 2 or meta.get("TotalNumVgprs", 999) > 256]
    if len(pairs) != 8 or bad:  # R3 = 10 / 12 x EXACT x TWIST (the twisted tiles' pass shape)
        print("kAnalyseTeamPairs budgets (eight instantiations, no scratch, two waves per SIMD, <= 256 registers): %d instantiation(s); %s" % (len(pairs), "; ".join(bad) or "none over budget"))
        return 1
    print("kAnalyseTeamPairs budgets: 8 instantiations, no scratch, two waves per SIMD, %s VGPRs" % " / ".join(str(meta["TotalNumVgprs"]) for _, meta in pairs))
    return 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--check-budgets"]:
        sys.exit(check_budgets(sys.argv[2]))
    for p in sys.argv[1:]:
        table(p)
