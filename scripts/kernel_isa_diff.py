#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, function by function (no GPU needed).

    scripts/kernel_isa_diff.py OLD_TREE NEW_TREE [--rename 'REGEX=>REPLACEMENT']... [--jobs N] [--keep DIR [--reuse]]

For each tree: rtc_feat.hip for every variant id of its csrc/Makefile, rtc_kernels.hip and, where the tree has them,
rtc_camera.hip, rtc_adaptive.hip, rtc_filter.hip, rtc_shutter.hip, rtc_background.hip (once plain, once per BG build id) and rtc_bump.hip (once plain, once per NP build id) are compiled to device-only assembly with that Makefile's FLAGS.  The assembly is split per function; comments, directives and label definitions
are dropped, local label references (.LBB<fn>_<n> ...) lose their function number, the function's own symbol becomes
<self>; what remains is counted and hashed.  Printed per function of NEW_TREE: unit, demangled name, instruction
count, hash, next_free_vgpr, next_free_sgpr, private segment size (device functions that are not kernels: the
NumVgprs / NumSgprs / ScratchSize the compiler reports), and SAME / DIFF against OLD_TREE's function of that name.
--rename rewrites OLD_TREE's demangled names (first matching rule only) for functions whose name is meant to change.
A function only one tree has is ONLY-OLD / ONLY-NEW.  Exit status 1 unless every line is SAME.
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("ARCH", "gfx950")
CSRC = os.path.join("raytracer_challenge_amd", "csrc")


def make_var(makefile, *names):
    for name in names:
        m = re.search(r"^%s\s*[:?]?=\s*(.*)$" % re.escape(name), makefile, re.M)
        if m and "$" not in m.group(1):
            return m.group(1).split()
    raise SystemExit("no %s in the Makefile" % " / ".join(names))


def units(tree):
    mk = open(os.path.join(tree, CSRC, "Makefile")).read()
    flags = make_var(mk, "FLAGS")
    out = [("feat%s" % v, "rtc_feat.hip", flags + ["-DRTC_VARIANT=%s" % v]) for v in make_var(mk, "VARIANT_IDS", "VARIANTS")]
    out.append(("kernels", "rtc_kernels.hip", flags))
    for unit, src in (("camera", "rtc_camera.hip"), ("adaptive", "rtc_adaptive.hip"), ("filter", "rtc_filter.hip"), ("shutter", "rtc_shutter.hip")):   # the small kernels beside the ray kernels, where a tree has them
        if os.path.exists(os.path.join(tree, CSRC, src)):
            out.append((unit, src, flags))
    if os.path.exists(os.path.join(tree, CSRC, "rtc_background.hip")):   # the background's kernels, and one unit per BG build of the one-kernel path
        out.append(("background", "rtc_background.hip", flags))
        out += [("background%s" % b, "rtc_background.hip", flags + ["-DRTC_BG_BUILD=%s" % b]) for b in make_var(mk, "BG_BUILD_IDS")]
    if os.path.exists(os.path.join(tree, CSRC, "rtc_bump.hip")):   # the bump records' kernel, and one unit per NP build of the one-kernel path
        out.append(("bump", "rtc_bump.hip", flags))
        out += [("bump%s" % b, "rtc_bump.hip", flags + ["-DRTC_NP_BUILD=%s" % b]) for b in make_var(mk, "NP_BUILD_IDS")]
    return out


def compile_unit(tree, unit, src, flags, outdir, reuse):
    out = os.path.join(outdir, unit + ".s")
    if reuse and os.path.exists(out):
        return unit, out
    cmd = [HIPCC, "--offload-arch=" + ARCH] + flags + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise SystemExit("%s\n%s" % (" ".join(cmd), r.stdout))
    return unit, out


def demangle(names):
    r = subprocess.run([os.environ.get("CXXFILT", "c++filt")], input="\n".join(names) + "\n", stdout=subprocess.PIPE, text=True, check=True)
    out = {}
    for n, d in zip(names, r.stdout.splitlines()):
        d = d.replace("(anonymous namespace)", "{anon}")
        out[n] = re.sub(r"^void ", "", d.split("(")[0])
    return out


def split_functions(path):
    """{mangled name: (n_instr, hash, vgpr, sgpr, scratch)}"""
    funcs, cur, body, info, in_code = {}, None, [], {}, False

    def close():
        if cur is None:
            return
        text = "\n".join(body).replace(cur, "<self>")
        funcs[cur] = (len(body), hashlib.sha1(text.encode()).hexdigest()[:12], info.get("vgpr", "-"), info.get("sgpr", "-"), info.get("scratch", "-"))

    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            close()
            cur, body, info, in_code = m.group(1), [], {}, True
            continue
        if cur is None:
            continue
        for key, pat in (("vgpr", r"\.amdhsa_next_free_vgpr\s+(\d+)"), ("sgpr", r"\.amdhsa_next_free_sgpr\s+(\d+)"), ("scratch", r"\.amdhsa_private_segment_fixed_size\s+(\d+)"),
                         ("vgpr", r";\s*NumVgprs:\s*(\d+)"), ("sgpr", r";\s*NumSgprs:\s*(\d+)"), ("scratch", r";\s*ScratchSize:\s*(\d+)")):
            m = re.search(pat, line)
            if m:
                info.setdefault(key, m.group(1))
        if re.match(r"\.Lfunc_end\d+:", line):
            in_code = False  # (the kernel descriptor and the compiler's summary comments follow)
        code = line.split(";")[0].strip()
        if not in_code or not code or code.startswith(".") or code.endswith(":"):
            continue
        body.append(re.sub(r"\.L([A-Za-z_]+)\d+_(\d+)", r".L\1_\2", " ".join(code.split())))
    close()
    return funcs


def analyse(tree, jobs, outdir, reuse):
    os.makedirs(outdir, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
        done = list(ex.map(lambda u: compile_unit(tree, u[0], u[1], u[2], outdir, reuse), units(tree)))
    table = {}
    for unit, path in done:
        funcs = split_functions(path)
        names = demangle(list(funcs))
        for mangled, row in funcs.items():
            table[(unit, names[mangled])] = row
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=>REPL", help="rewrite a demangled name of OLD_TREE (re.fullmatch; first matching rule only)")
    ap.add_argument("--jobs", type=int, default=8, help="compiler processes at a time (at most 16)")
    ap.add_argument("--keep", help="directory for the assembly files (default: a temporary one)")
    ap.add_argument("--reuse", action="store_true", help="with --keep: do not recompile a unit whose assembly file is already there")
    a = ap.parse_args()
    jobs = max(1, min(16, a.jobs))
    rules = [tuple(r.split("=>", 1)) for r in a.rename]

    def renamed(name):
        for pat, repl in rules:
            if re.fullmatch(pat, name):
                return re.sub(pat, repl, name)
        return name

    with tempfile.TemporaryDirectory() as tmp:
        base = a.keep or tmp
        old = {(u, renamed(n)): row for (u, n), row in analyse(a.old_tree, jobs, os.path.join(base, "old"), a.reuse).items()}
        new = analyse(a.new_tree, jobs, os.path.join(base, "new"), a.reuse)
    for pat, repl in rules:
        print("# rename: %s => %s" % (pat, repl))
    print("# %-8s %9s %-12s %5s %5s %8s  %-8s %s" % ("unit", "instr", "hash", "vgpr", "sgpr", "scratch", "", "function"))
    bad = 0
    for key in sorted(set(old) | set(new)):
        row = new.get(key) or old[key]
        verdict = "ONLY-OLD" if key not in new else "ONLY-NEW" if key not in old else "SAME" if old[key] == new[key] else "DIFF"
        bad += verdict != "SAME"
        print("%-10s %9d %-12s %5s %5s %8s  %-8s %s" % (key[0], row[0], row[1], row[2], row[3], row[4], verdict, key[1]))
        if verdict == "DIFF":
            print("%-10s %9d %-12s %5s %5s %8s  %-8s %s" % ("", *old[key], "(old)", ""))
    print("# %d functions, %d not SAME" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
