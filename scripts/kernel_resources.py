#!/usr/bin/env python3
"""Register / scratch / LDS use of every kernel of a csrc/*.hip file, from hipcc's
-Rpass-analysis=kernel-resource-usage (cross-compiles: no GPU needed).

    python3 scripts/kernel_resources.py bm25_walk_block [-DNAME ...]    # one unit, or `all`

--isa: one line per kernel of the unit(s) -- mangled name, a hash of its instructions, VGPR / AGPR /
scratch / LDS, the unit that defines it -- for proving that a change which only MOVES kernels between
files left every one of them as it was.  The hash covers the body from the kernel's label to its
.Lfunc_end, without comments and directives and with the function index taken out of the local labels
(.LBB<n>_ -> .LBB_), so it does not depend on the kernel's position in its file.

    python3 scripts/kernel_resources.py --isa all > before.txt          # on the old tree
    python3 scripts/kernel_resources.py --isa all --against before.txt  # on the new one: exit 1 on any difference
"""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bases(arg):
    import triple_hybrid_rag_amd as T
    if arg != "all":
        return [arg]
    return [os.path.basename(s)[:-4] for s in T._build.sources()]


def resources(base, defines=()):
    import triple_hybrid_rag_amd as T
    src = os.path.join(T._build.CSRC, base + ".hip")
    cmd = ["/opt/rocm/bin/hipcc"] + T._build.HIPCC_FLAGS + list(defines) + \
          ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", "/dev/null"]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            name = text.split(":", 1)[1].strip()
            demangled = subprocess.run(["c++filt", name], capture_output=True,
                                       text=True).stdout.strip()
            cur = {"kernel": re.sub(r"\(.*", "", demangled).replace("void thr::", "")}
            out.append(cur)
        elif cur is not None and ":" in text:
            k, v = text.split(":", 1)
            cur[k.strip()] = v.strip()
    return out


def isa(base, defines=()):
    """{mangled kernel name: (hash, instructions, vgpr, agpr, scratch, lds, base)} of one unit."""
    import triple_hybrid_rag_amd as T
    src = os.path.join(T._build.CSRC, base + ".hip")
    cmd = ["/opt/rocm/bin/hipcc"] + T._build.HIPCC_FLAGS + list(defines) + \
          ["--cuda-device-only", "-S", src, "-o", "-"]
    txt = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout.split("\n")
    label = {m.group(1): i for i, l in enumerate(txt) for m in [re.match(r"([A-Za-z_]\S*):", l)] if m}
    out = {}
    for name in [l.split()[1] for l in txt if l.strip().startswith(".amdhsa_kernel ")]:
        body, end = [], None
        for i in range(label[name] + 1, len(txt)):
            s = re.sub(r"\s*;.*$", "", txt[i].strip())
            if s.startswith(".Lfunc_end"):
                end = i
                break
            s = re.sub(r"\.LBB\d+_", ".LBB_", s)
            if s and (not s.startswith(".") or s.startswith(".LBB_")):
                body.append(s)
        info = {}
        for l in txt[end:end + 60]:   # the "; Kernel info:" block that follows the function
            m = re.match(r";\s*(NumVgprs|NumAgprs|ScratchSize|LDSByteSize):\s*(\d+)", l)
            if m:
                info.setdefault(m.group(1), m.group(2))
        out[name] = (hashlib.sha1("\n".join(body).encode()).hexdigest()[:16], str(len(body)),
                     info["NumVgprs"], info["NumAgprs"], info["ScratchSize"], info["LDSByteSize"], base)
    return out


def isa_table(which, defines=()):
    """The table of every unit of `which`; a kernel defined in two units is an error."""
    table, twice = {}, []
    with ThreadPoolExecutor(max_workers=min(16, int(os.environ.get("MAX_JOBS", 16)))) as ex:
        for unit in ex.map(lambda b: isa(b, defines), bases(which)):
            twice += [k for k in unit if k in table]
            table.update(unit)
    if twice:
        sys.exit("defined in more than one unit: " + " ".join(twice))
    return table


def isa_main(argv):
    against = None
    if "--against" in argv:
        i = argv.index("--against")
        against = argv[i + 1]
        del argv[i:i + 2]
    table = isa_table(argv[0], argv[1:])
    for name in sorted(table):
        print(name, *table[name])
    if against is None:
        return 0
    old = {l.split()[0]: tuple(l.split()[1:]) for l in open(against) if l.strip()}
    bad = 0
    for name in sorted(set(old) | set(table)):
        a, b = old.get(name), table.get(name)
        if a is None or b is None or a[:6] != b[:6]:   # (the unit, the last column, may change)
            print("DIFFERS", name, a, b, file=sys.stderr)
            bad += 1
    print(f"{len(table)} kernels, {len(old)} in {against}, {bad} differ", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--isa":
        sys.exit(isa_main(sys.argv[2:]))
    for base in bases(sys.argv[1]):
        for r in resources(base, sys.argv[2:]):
            print(f"{r['kernel'][:70]:70s} VGPR {r.get('VGPRs'):>4s} AGPR {r.get('AGPRs'):>3s} "
                  f"spill {r.get('VGPR Spill', r.get('VGPRs Spill', '?')):>3s} scratch {r.get('ScratchSize [bytes/lane]'):>4s} "
                  f"occ {r.get('Occupancy [waves/SIMD]'):>2s} LDS {r.get('LDS Size [bytes/block]')}")
