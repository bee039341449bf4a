#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, function by function (no GPU needed).

    scripts/kernel_isa_diff.py OLD_TREE NEW_TREE [--rename 'REGEX=>REPLACEMENT']... [--unit OLD=NEW]... [--jobs N] [--keep DIR [--reuse]]

The units of a tree are those of its csrc/Makefile: every source that is built once per id of a list ($(foreach v,$(IDS),$(O)/<name>$(v).o)
with a rule `$(O)/<name>%.o: <source>` that passes -D<WHAT>=$*: rtc_feat.hip per row of VARIANT_IDS, unit feat<row>; in earlier layouts
also units background<b> and bump<b>); rtc_feat.hip for every row of GENERAL_IDS and extension of EXT_IDS (-DRTC_VARIANT -DRTC_EXT: unit
feat<row>_ext<e>); and the small units, SMALL_UNITS or every `$(O)/<name>.o: <name>.hip` rule.  Each is compiled to device-only assembly with that Makefile's FLAGS.  The assembly is split
per function; comments, directives and label definitions are dropped, local label references (.LBB<fn>_<n> ...) lose their function
number, .Lpost_getpc<n> labels (numbered per translation unit by the compiler) are renumbered per function in order of appearance, the
function's own symbol becomes <self>; what remains is counted and hashed.  Printed per function of NEW_TREE: unit, demangled name,
instruction count, hash, next_free_vgpr, next_free_sgpr, private segment size (device functions that are not kernels: the
NumVgprs / NumSgprs / ScratchSize the compiler reports), and SAME / DIFF against OLD_TREE's function of that name.
--rename rewrites OLD_TREE's demangled names (first matching rule only) for functions whose name is meant to change.
--unit says that OLD_TREE's unit OLD is NEW_TREE's unit NEW, for functions that moved to another translation unit.
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


def make_var_or(makefile, name, default=None):
    try:
        return make_var(makefile, name)
    except SystemExit:
        return default


def units(tree):
    mk = open(os.path.join(tree, CSRC, "Makefile")).read()
    flags = make_var(mk, "FLAGS")
    out = []
    # one object per id of a list: $(foreach v,$(IDS),$(O)/<name>$(v).o) in OBJS, built by the rule `$(O)/<name>%.o: <src>` with -D<WHAT>=$*
    for m in re.finditer(r"\$\(foreach (\w+),\$\((\w+)\),\$\(O\)/(\w+)\$\(\1\)\.o\)", mk):
        ids, name = make_var_or(mk, m.group(2)), m.group(3)
        rule = re.search(r"^\$\(O\)/%s%%\.o: (\S+\.hip).*\n\t.*?(-D\w+)=\$\*" % name, mk, re.M)
        if ids and rule:
            out += [(re.sub(r"^rtc_", "", name) + v, rule.group(1), flags + ["%s=%s" % (rule.group(2), v)]) for v in ids]
    for v in make_var_or(mk, "GENERAL_IDS") or []:   # the extended one-kernel builds: a general row x an extension
        out += [("feat%s_ext%s" % (v, e), "rtc_feat.hip", flags + ["-DRTC_VARIANT=%s" % v, "-DRTC_EXT=%s" % e]) for e in make_var(mk, "EXT_IDS")]
    small = make_var_or(mk, "SMALL_UNITS") or [m.group(1) for m in re.finditer(r"^\$\(O\)/(\w+)\.o: \1\.hip", mk, re.M)]
    out += [(re.sub(r"^rtc_", "", name), name + ".hip", flags) for name in small]
    if not any(u[0].startswith("feat") for u in out):
        raise SystemExit("no rtc_feat objects in %s's Makefile" % tree)
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
    funcs, cur, body, info, in_code, getpc = {}, None, [], {}, False, {}

    def close():
        if cur is None:
            return
        text = "\n".join(body).replace(cur, "<self>")
        funcs[cur] = (len(body), hashlib.sha1(text.encode()).hexdigest()[:12], info.get("vgpr", "-"), info.get("sgpr", "-"), info.get("scratch", "-"))

    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            close()
            cur, body, info, in_code, getpc = m.group(1), [], {}, True, {}
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
        code = re.sub(r"\.L([A-Za-z_]+)\d+_(\d+)", r".L\1_\2", " ".join(code.split()))
        body.append(re.sub(r"\.Lpost_getpc(\d+)", lambda m: ".Lpost_getpc#%d" % getpc.setdefault(m.group(1), len(getpc)), code))
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
    ap.add_argument("--unit", action="append", default=[], metavar="OLD=NEW", help="OLD_TREE's unit OLD corresponds to NEW_TREE's unit NEW")
    ap.add_argument("--jobs", type=int, default=8, help="compiler processes at a time (at most 16)")
    ap.add_argument("--keep", help="directory for the assembly files (default: a temporary one)")
    ap.add_argument("--reuse", action="store_true", help="with --keep: do not recompile a unit whose assembly file is already there")
    a = ap.parse_args()
    jobs = max(1, min(16, a.jobs))
    rules = [tuple(r.split("=>", 1)) for r in a.rename]
    moved = dict(u.split("=", 1) for u in a.unit)

    def renamed(name):
        for pat, repl in rules:
            if re.fullmatch(pat, name):
                return re.sub(pat, repl, name)
        return name

    with tempfile.TemporaryDirectory() as tmp:
        base = a.keep or tmp
        old = {(moved.get(u, u), renamed(n)): row for (u, n), row in analyse(a.old_tree, jobs, os.path.join(base, "old"), a.reuse).items()}
        new = analyse(a.new_tree, jobs, os.path.join(base, "new"), a.reuse)
    for pat, repl in rules:
        print("# rename: %s => %s" % (pat, repl))
    for u, v in moved.items():
        print("# unit: %s => %s" % (u, v))
    print("# %-11s %9s %-12s %5s %5s %8s  %-8s %s" % ("unit", "instr", "hash", "vgpr", "sgpr", "scratch", "", "function"))
    bad = 0
    for key in sorted(set(old) | set(new)):
        row = new.get(key) or old[key]
        verdict = "ONLY-OLD" if key not in new else "ONLY-NEW" if key not in old else "SAME" if old[key] == new[key] else "DIFF"
        bad += verdict != "SAME"
        print("%-13s %9d %-12s %5s %5s %8s  %-8s %s" % (key[0], row[0], row[1], row[2], row[3], row[4], verdict, key[1]))
        if verdict == "DIFF":
            print("%-13s %9d %-12s %5s %5s %8s  %-8s %s" % ("", *old[key], "(old)", ""))
    print("# %d functions, %d not SAME" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
