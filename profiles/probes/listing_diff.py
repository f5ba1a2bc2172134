"""Are the stream kernels' device listings the same in two source trees?  (No GPU needed.)

    python profiles/probes/listing_diff.py PARENT_TREE BRANCH_TREE [--work DIR] [--reuse] [--jobs N]

Compiles, in both trees, every unit of build.py's DEVICE_UNITS that is built from a stream source (ranked_stream.hip,
ranked_stream_mixed.hip, union_stream.hip: the plain, _bigk and _docs builds) with build.py's COMMON flags plus
`-S --cuda-device-only`, and the three sources once more under each diagnostic flag (-DDS2I_RS_PHASE, -DDS2I_US_PHASE,
-DDS2I_LINE_COUNT). The two listings of a unit are then compared kernel by kernel: the set of names, every kernel's
instruction sequence (comments dropped, local labels renumbered in order of appearance), its .amdhsa_* values, the
metadata, and whatever else the listing holds. Lines naming the per-compilation `__hip_cuid_*` symbol are ignored.
A refactor that only moves device helpers between files must leave all of them identical; exit status 1 if one is not.
The units and flags are read from BRANCH_TREE's build.py. --work keeps the listings (parent/ and branch/ below it);
--reuse skips a compilation whose listing is already there (the parent's, between two attempts at the branch).
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

STREAM_SOURCES = ("ranked_stream.hip", "ranked_stream_mixed.hip", "union_stream.hip")
DIAGNOSTIC_FLAGS = ("-DDS2I_RS_PHASE", "-DDS2I_US_PHASE", "-DDS2I_LINE_COUNT")
LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def load_build(tree):
    spec = importlib.util.spec_from_file_location("ds2i_build_py", os.path.join(tree, "ds2i_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def units_of(build):
    units = [(src, name.replace(".hip", ""), defs) for src, name, defs in build.DEVICE_UNITS if src in STREAM_SOURCES]
    for src in STREAM_SOURCES:
        for flag in DIAGNOSTIC_FLAGS:
            units.append((src, src.replace(".hip", "") + "." + flag[len("-DDS2I_"):].lower(), [flag]))
    return units


def compile_listing(build, tree, src, defs, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=" + build.ARCH] + build.COMMON + defs + ["-S", "--cuda-device-only",
           os.path.join(tree, "ds2i_amd", "csrc", src), "-o", out]
    subprocess.check_call(cmd)


def parse(text):
    """-> {"kernel <name>": lines, "amdhsa <name>": lines, "metadata": lines, "rest": lines}"""
    parts = {"metadata": [], "rest": []}
    cur = parts["rest"]
    pending, labels = None, {}
    for raw in text.splitlines():
        if "__hip_cuid_" in raw:
            continue
        line = raw.split(";", 1)[0].strip()
        if not line or line.startswith((".ident", ".file")):
            continue
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            pending = m.group(1)
        elif pending and line == pending + ":":
            cur, labels, pending = parts.setdefault("kernel " + line[:-1], []), {}, None
            continue
        elif line.startswith(".Lfunc_end"):
            cur = parts["rest"]
            continue
        elif line.startswith(".amdhsa_kernel "):
            cur = parts.setdefault("amdhsa " + line.split()[1], [])
            continue
        elif line == ".end_amdhsa_kernel":
            cur = parts["rest"]
            continue
        elif line == ".amdgpu_metadata":
            cur = parts["metadata"]
            continue
        elif line == ".end_amdgpu_metadata":
            cur = parts["rest"]
            continue
        if cur is not parts["metadata"]:
            line = LOCAL_LABEL.sub(lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), line)
        cur.append(line)
    return parts


def differences(a, b):
    out = []
    for key in sorted(set(a) | set(b)):
        if key not in a or key not in b:
            out.append("%s: only in the %s" % (key, "parent" if key in a else "branch"))
        elif a[key] != b[key]:
            n = sum(1 for x, y in zip(a[key], b[key]) if x != y) + abs(len(a[key]) - len(b[key]))
            out.append("%s: %d of %d lines differ" % (key, n, max(len(a[key]), len(b[key]))))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--work", default=None)
    ap.add_argument("--reuse", action="store_true")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 4))
    args = ap.parse_args()
    work = args.work or tempfile.mkdtemp(prefix="listing_diff_")
    build = load_build(args.branch)
    units = units_of(build)
    jobs = []
    for side, tree in (("parent", args.parent), ("branch", args.branch)):
        os.makedirs(os.path.join(work, side), exist_ok=True)
        for src, name, defs in units:
            out = os.path.join(work, side, name + ".s")
            if not (args.reuse and os.path.exists(out)):
                jobs.append((build, tree, src, defs, out))
    with ThreadPoolExecutor(max_workers=max(1, args.jobs)) as pool:
        list(pool.map(lambda j: compile_listing(*j), jobs))
    bad = 0
    for src, name, defs in units:
        sides = [parse(open(os.path.join(work, side, name + ".s")).read()) for side in ("parent", "branch")]
        diff = differences(*sides)
        kernels = sum(1 for k in sides[1] if k.startswith("kernel "))
        print("%-40s %s" % (name, "identical (%d kernels)" % kernels if not diff else "DIFFERS"))
        for d in diff:
            print("    " + d)
        bad += bool(diff)
    print("%d of %d units differ" % (bad, len(units)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
