"""Kernel resource tables from the build logs (hipcc -Rpass-analysis=kernel-resource-usage, build/obj/*.log).

    python tools/kernel_resources.py LOGDIR                 every kernel: SGPRs, VGPRs, AGPRs, scratch, occupancy, LDS
    python tools/kernel_resources.py LOGDIR --against OLD   the kernels whose figures differ from OLD's, and the ones only one side has

Names are demangled with c++filt when it is there.  Exit status 1 when --against finds a kernel of OLD whose figures moved.
"""
import os
import re
import subprocess
import sys

FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds"))


def parse(logdir):
    out = {}
    for f in sorted(os.listdir(logdir)):
        if not f.endswith(".log"):
            continue
        cur = None
        for line in open(os.path.join(logdir, f), errors="ignore"):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = out.setdefault((f.split(".")[0], m.group(1)), {})
                continue
            if cur is None:
                continue
            for label, key in FIELDS:
                m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
                if m:
                    cur[key] = int(m.group(1))
    return out


def demangle(names):
    try:
        txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, txt))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*$", "", name)  # the argument list
    return name.replace("amsm::", "")


def row(unit, name, r):
    return f"{unit:<16} {name:<72} " + " ".join(f"{k}={r.get(k, '?')}" for _, k in FIELDS)


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    new = parse(sys.argv[1])
    dm = demangle(sorted({n for _, n in new}))
    if "--against" not in sys.argv:
        for (unit, n), r in sorted(new.items()):
            print(row(unit, short(dm[n]), r))
        return
    old = parse(sys.argv[sys.argv.index("--against") + 1])
    dm.update(demangle(sorted({n for _, n in old})))
    moved = 0
    for key in sorted(set(old) | set(new)):
        unit, n = key
        if key not in new:
            print("GONE   ", row(unit, short(dm[n]), old[key]))
            moved += 1
        elif key not in old:
            print("NEW    ", row(unit, short(dm[n]), new[key]))
        elif old[key] != new[key]:
            print("MOVED  ", row(unit, short(dm[n]), old[key]))
            print("    ->  ", row(unit, short(dm[n]), new[key]))
            moved += 1
    print(f"{len(old)} kernels before, {len(new)} now, {moved} moved or gone")
    sys.exit(1 if moved else 0)


if __name__ == "__main__":
    main()
