"""Register, scratch, occupancy and LDS figures of every kernel of some units, from the compiler alone (no GPU): the units are compiled with build.py's
flags plus -Rpass-analysis=kernel-resource-usage and the remarks are tabulated. The flag list below is a COPY of build_hip's compile line (without the
WH_PROBES define): keep it in step when build.py changes.

    python tools/kernel_resources.py elementwise.hip sample.hip beam.hip [--root OTHER_CHECKOUT] [--against OTHER_CHECKOUT]

--against prints the two trees side by side, one row per kernel, and exits 1 when a kernel differs in one of the six columns (VGPRs, AGPRs, scratch bytes
per lane, VGPR spills, occupancy, LDS bytes); SGPR spills are shown and not compared. A unit that one of the trees does not have contributes no kernels
there, so kernels that moved between units are compared by name."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisper_amd import build as B  # noqa: E402

FIELDS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("VGPRs Spill", "vspill"), ("Occupancy [waves/SIMD]", "occ"),
          ("LDS Size [bytes/block]", "lds"), ("SGPRs Spill", "sspill")]
COMPARED = [short for _, short in FIELDS[:6]]


def short_name(mangled):
    # (_Float16 is a builtin type older demanglers do not know: spelled as `half` for the name's sake)
    name = subprocess.run(["c++filt", mangled.replace("DF16_", "Dh")], stdout=subprocess.PIPE, text=True).stdout.strip()
    name = re.sub(r"^void ", "", name).replace("wh::(anonymous namespace)::", "")
    depth = 0
    for i, ch in enumerate(name):           # cut the argument list: the first '(' outside the template arguments
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def resources(root, units):
    out = {}
    for u in units:
        if not os.path.exists(os.path.join(root, "whisper_amd", "csrc", u)):
            continue                        # a unit one tree does not have (a kernel moved between units): no kernels from it
        cmd = [B.HIPCC, "--offload-arch=" + B.ARCH, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wno-unused-result"] + B.EXTRA_FLAGS.get(u, []) + \
              ["-I" + os.path.join(root, "include"), "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(root, "whisper_amd", "csrc", u), "-o", os.devnull]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.exit(r.stdout)
        cur = None
        for line in r.stdout.splitlines():
            m = re.search(r"remark: .*Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(short_name(m.group(1)), {})
                continue
            for key, short in FIELDS:
                m = re.search(r"remark: .*\s" + re.escape(key) + r": (\d+)", line)
                if m and cur is not None:
                    cur[short] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("units", nargs="+")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--against", default="", help="a second checkout (the parent commit): its kernels in the left columns")
    a = ap.parse_args()
    cols = [short for _, short in FIELDS]
    head = resources(a.root, a.units)
    base = resources(a.against, a.units) if a.against else None
    fmt = "%-34s" + ("  " + " %7s" * len(cols)) * (2 if base else 1)
    if base:
        print(fmt % (("", ) + ("parent", ) + ("", ) * (len(cols) - 1) + ("head", ) + ("", ) * (len(cols) - 1)) + "   equal")
    print(fmt % (("kernel", ) + tuple(cols) * (2 if base else 1)))
    bad = 0
    for k in sorted(set(head) | set(base or {})):
        h = tuple(head.get(k, {}).get(c, "-") for c in cols)
        if not base:
            print(fmt % ((k, ) + h))
            continue
        b = tuple(base.get(k, {}).get(c, "-") for c in cols)
        same = all(head.get(k, {}).get(c) == base.get(k, {}).get(c) for c in COMPARED) and k in head and k in base
        bad += not same
        print(fmt % ((k, ) + b + h) + "   " + ("yes" if same else "NO"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
