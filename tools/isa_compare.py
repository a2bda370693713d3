#!/usr/bin/env python3
"""isa_compare.py PARENT_CSRC THIS_CSRC [-o TABLE] — do two trees' vmx_kernels.hip compile to the same gfx950 code?

Compiles vmx_kernels.hip of both csrc directories with their own Makefile's flags plus `--cuda-device-only -S`, splits
the assembly per kernel symbol, normalises local labels and reports, per kernel:
  a. whether the instruction text is identical,
  b. next_free_vgpr, next_free_sgpr, group_segment_fixed_size and private_segment_fixed_size of both sides,
  c. the opcode histogram difference, the _e32 / _e64 encoding suffix stripped.
It only compares two builds; it needs no GPU.  PARENT_CSRC is the csrc directory of a `git worktree` or `git archive`
export of the commit to compare against.

The verdict per kernel is `same` (identical text), `ok` or `FAIL`.  A kernel of the image-space passes (the kernels of
vmx_filter.inc, vmx_variance.inc, vmx_upsample.inc and vmx_temporal.inc) is `ok` if its VGPRs and SGPRs are not higher,
its LDS is equal, its scratch is 0, its histogram is equal for every opcode that starts v_, ds_, global_, buffer_ or
flat_, and its instruction count is within +-2; every other kernel must be `same`.  Exit status 1 if any is FAIL.
"""
import argparse
import collections
import concurrent.futures
import pathlib
import re
import subprocess
import sys
import tempfile

# the image-space kernels, as their names start once mangled (namespace vmx, <length><name>)
IMAGE = ("_ZN3vmx14k_filter_guideE", "_ZN3vmx14k_demod_divideI", "_ZN3vmx8k_atrousI", "_ZN3vmx12k_atrous_varI",
         "_ZN3vmx10k_varianceI", "_ZN3vmx15k_variance_packI", "_ZN3vmx10k_upsampleI", "_ZN3vmx10k_temporalI")
VECTOR = ("v_", "ds_", "global_", "buffer_", "flat_")
FIELDS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def makefile_flags(csrc):
    """(hipcc, flags) as csrc/Makefile's defaults give them"""
    text = (csrc / "Makefile").read_text()
    var = dict(re.findall(r"^(\w+) \?= ?(.*)$", text, re.M))
    flags = re.search(r"^CXXFLAGS := (.*)$", text, re.M).group(1)
    flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), flags)
    return var["HIPCC"], ["--offload-arch=" + var["ARCH"]] + flags.split()


def assembly(csrc, out):
    hipcc, flags = makefile_flags(csrc)
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), "vmx_kernels.hip"], cwd=csrc, check=True)
    return out.read_text()


def kernels(asm):
    """{symbol: (instruction lines, {field: value})} of every .amdhsa_kernel in the text"""
    lines = asm.splitlines()
    start = {m.group(1): i for i, s in enumerate(lines) if (m := re.match(r"^([A-Za-z_][\w$.]*):", s))}
    out = {}
    for i, s in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", s)
        if not m:
            continue
        sym, meta = m.group(1), {}
        for t in lines[i:]:
            if ".end_amdhsa_kernel" in t:
                break
            f = re.match(r"\s*\.amdhsa_(\w+) (\d+)", t)
            if f and f.group(1) in FIELDS:
                meta[f.group(1)] = int(f.group(2))
        body = []
        for t in lines[start[sym] + 1:]:
            if t.startswith(".Lfunc_end"):
                break
            t = t.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.endswith(":")):
                continue  # comments and directives; labels stay
            body.append(re.sub(r"\.L(BB|tmp|JTI)\d+_", r".L\1_", t))
        out[sym] = (body, meta)
    return out


def histogram(body):
    ops = (t.split()[0] for t in body if not t.endswith(":"))
    return collections.Counter(re.sub(r"_e(32|64)$", "", o) for o in ops)


def compare(parent, this):
    rows, bad = [], 0
    for sym in sorted(set(parent) | set(this)):
        if sym not in parent or sym not in this:
            rows.append(f"FAIL  {sym}: only in {'this' if sym in this else 'parent'}")
            bad += 1
            continue
        (pb, pm), (tb, tm) = parent[sym], this[sym]
        ph, th = histogram(pb), histogram(tb)
        diff = {o: th[o] - ph[o] for o in sorted(set(ph) | set(th)) if th[o] != ph[o]}
        n_p, n_t = sum(ph.values()), sum(th.values())
        image = sym.startswith(IMAGE)
        if pb == tb and pm == tm:
            verdict = "same"
        elif image and tm["next_free_vgpr"] <= pm["next_free_vgpr"] and tm["next_free_sgpr"] <= pm["next_free_sgpr"] \
                and tm["group_segment_fixed_size"] == pm["group_segment_fixed_size"] \
                and tm["private_segment_fixed_size"] == 0 and abs(n_t - n_p) <= 2 \
                and not any(o.startswith(VECTOR) for o in diff):
            verdict = "ok"
        else:
            verdict = "FAIL"
            bad += 1
        regs = " ".join(f"{n} {pm[f]}/{tm[f]}" for n, f in zip(("vgpr", "sgpr", "lds", "scratch"), FIELDS))
        rows.append(f"{verdict:5s} {'image' if image else 'other'} {sym}: {regs} insts {n_p}/{n_t}"
                    + (" diff " + " ".join(f"{o}{d:+d}" for o, d in diff.items()) if diff else ""))
    return rows, bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("parent_csrc", type=pathlib.Path)
    ap.add_argument("this_csrc", type=pathlib.Path)
    ap.add_argument("-o", "--out", type=pathlib.Path, help="also write the table here")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=TEXT",
                    help="a kernel whose signature changed: the parent's symbols are compared under the name re.sub gives them")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(2) as pool:
        jobs = [pool.submit(assembly, d.resolve(), pathlib.Path(tmp) / f"{n}.s")
                for n, d in (("parent", a.parent_csrc), ("this", a.this_csrc))]
        parent, this = (kernels(j.result()) for j in jobs)
    for r in a.rename:
        pat, text = r.split("=", 1)
        parent = {re.sub(pat, text, sym): v for sym, v in parent.items()}
    rows, bad = compare(parent, this)
    n_image = sum(" image " in r for r in rows)
    head = [f"# tools/isa_compare.py: {len(rows)} kernels, {n_image} image-space; parent/this per figure",
            f"# same {sum(r.startswith('same') for r in rows)}, ok {sum(r.startswith('ok') for r in rows)}, FAIL {bad}"]
    text = "\n".join(head + rows) + "\n"
    sys.stdout.write(text)
    if a.out:
        a.out.write_text(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
