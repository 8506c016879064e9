#!/usr/bin/env python3
"""Compare the gfx950 kernels of two sets of HIP translation units, kernel by kernel.

    tools/compare_kernels.py --old OLD.hip [...] --new NEW.hip [...] [--out TABLE.md]

Each unit is cross-compiled device-side to assembly text with the Makefile's HIPFLAGS and
-Rpass-analysis=kernel-resource-usage (no GPU is used). Kernels are matched by demangled name with
`(anonymous namespace)::` and `srt::` dropped, so a type that moved between the two namespaces still
matches. Per kernel the instruction text from its entry label to its function-end label (comments
dropped, the function number of local labels dropped) and the resource remarks must be equal. Prints
one table row per kernel; exit status 1 if the sets differ or any kernel does.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")
# the Makefile's own HIPFLAGS (make print-hipflags), so the two cannot drift apart
HIPFLAGS = subprocess.run(["make", "-s", "-C", REPO, "print-hipflags"], stdout=subprocess.PIPE, text=True,
                          check=True).stdout.split()
RESOURCES = {"TotalSGPRs": "SGPRs", "VGPRs": "VGPRs", "AGPRs": "AGPRs", "ScratchSize [bytes/lane]": "scratch",
             "SGPRs Spill": "SGPR spill", "VGPRs Spill": "VGPR spill", "LDS Size [bytes/block]": "LDS",
             "Occupancy [waves/SIMD]": "occupancy"}


def compile_unit(src, tmp, extra):
    asm = os.path.join(tmp, os.path.basename(src) + "." + str(len(os.listdir(tmp))) + ".s")
    cmd = [HIPCC, *HIPFLAGS, *extra, "-I", os.path.join(REPO, "simpleraytracer_amd/csrc"), "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", os.path.abspath(src), "-o", asm]
    done = subprocess.run(cmd, cwd=REPO, stderr=subprocess.PIPE, text=True, check=True)
    return open(asm).read(), done.stderr


def normalise(text):
    text = subprocess.run([CXXFILT], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout
    text = text.replace("(anonymous namespace)::", "").replace("srt::", "")
    # what c++filt leaves mangled (_Float16 arguments): at least the kernel's own name, readable
    text = re.sub(r"_ZN3srt12_GLOBAL__N_1(\d+)(\w+)", lambda m: m.group(2)[:int(m.group(1))] + " [" + m.group(2)[int(m.group(1)):] + "]", text)
    return re.sub(r"\.L(BB|JTI|func_end|func_begin|tmp)\d+", r".L\1", text)


def kernels(sources, tmp, extra):
    """{normalised demangled name: (instruction lines, resource line)} of the units' kernels."""
    out = {}
    for src in sources:
        asm, remarks = compile_unit(src, tmp, extra)
        res, name = {}, None
        for line in remarks.splitlines():
            m = re.search(r"remark: +(Function Name|[A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
            if m and m.group(1) == "Function Name":
                name = m.group(2)
                res[name] = {}
            elif m and name is not None:
                res[name][m.group(1)] = m.group(2)
        lines = asm.splitlines()
        for mangled, r in res.items():
            begin = lines.index(next(l for l in lines if l.startswith(mangled + ":")))
            # the kernel's own end label, as its .size directive names it
            label = next(m.group(1) for m in (re.match(r"\s*\.size\s+" + re.escape(mangled) + r",\s*(\.Lfunc_end\d+)-", l)
                                              for l in lines[begin:]) if m)
            end = lines.index(label + ":", begin)
            body = [re.sub(r"\s*;.*$", "", l) for l in lines[begin:end + 1]]
            # (.section lines carry the kernel's mangled name, which holds the namespace of its argument types)
            body = normalise("\n".join(l for l in body if l.strip() and not l.lstrip().startswith(".section"))).splitlines()
            key = normalise(mangled).strip()
            assert key not in out, key
            out[key] = (body[1:], ", ".join(f"{label} {r[k]}" for k, label in RESOURCES.items() if r[k] != "0" or label in ("SGPRs", "VGPRs", "LDS")), os.path.basename(src))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--flags", default="", help="extra compiler flags for both sides, e.g. -DSRT_DIAG")
    ap.add_argument("--out", help="also write the table here")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(a.old, tmp, a.flags.split()), kernels(a.new, tmp, a.flags.split())
    rows = ["| kernel | unit | lines | text | resources | resource line |", "|---|---|---|---|---|---|"]
    bad = sorted(set(old) ^ set(new))
    for k in bad:
        rows.append(f"| `{k}` | {(old.get(k) or new.get(k))[2]} | - | only in {'old' if k in old else 'new'} | - | - |")
    for k in sorted(set(old) & set(new)):
        text, res = old[k][0] == new[k][0], old[k][1] == new[k][1]
        if not (text and res):
            bad.append(k)
        if not text:  # the first line that differs, for whoever has to find the edit
            at = next((i for i, (x, y) in enumerate(zip(old[k][0], new[k][0])) if x != y), min(len(old[k][0]), len(new[k][0])))
            print(f"{k}: line {at}: {old[k][0][at:at + 1]} -> {new[k][0][at:at + 1]}", file=sys.stderr)
        rows.append(f"| `{k}` | {new[k][2]} | {len(new[k][0])} | {'equal' if text else 'DIFFERS'} | "
                    f"{'equal' if res else 'DIFFERS: was ' + old[k][1]} | {new[k][1]} |")
    rows.append("")
    rows.append(f"{len(old)} kernels old, {len(new)} new, {len(bad)} unmatched or different.")
    table = "\n".join(rows) + "\n"
    sys.stdout.write(table)
    if a.out:
        open(a.out, "w").write(table)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
