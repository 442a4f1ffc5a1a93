"""Per-kernel ISA summary of a hipcc -save-temps .s file: VGPR/AGPR/scratch and instruction counts.

    python tools/isa_summary.py file.s [name-substring]
    python tools/isa_summary.py --diff old.s new.s [old_name=new_name ...]

--diff pairs every kernel of new.s with old.s's kernel of the same mangled name, or of the name a
pair on the command line gives for it (a template parameter that was folded away), and compares
the instruction streams (comments stripped, per-function label numbers collapsed) and the
register / scratch / occupancy / LDS lines.  Exit status 1 if any pair differs.
"""
import re
import sys

RESOURCES = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def kernels(path):
    """{mangled name: (function body, text of the resource block after it)}"""
    s = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\S+):\s*;\s*@", s, re.M):
        end = s.find(".Lfunc_end", m.end())
        out[m.group(1)] = (s[m.end():end], s[end:end + 3000])
    return out


def normalised(name, body):
    lines = []
    for ln in body.replace(name, "<kernel>").splitlines():
        ln = re.sub(r"\.(LBB|Ltmp|Lfunc_end)\d+", r".\1", ln.split(";")[0]).rstrip()
        if ln:
            lines.append(ln)
    return lines


def resources(info):
    return {k: (re.search(rf"; {k}: (\d+)", info) or [None, None])[1] for k in RESOURCES}


def diff(old_path, new_path, *pairs):
    old, new = kernels(old_path), kernels(new_path)
    old_of = {n: o for o, n in (p.split("=") for p in pairs)}
    bad = 0
    for name, (body, info) in new.items():
        oname = old_of.get(name, name)
        if oname not in old:
            print(f"NEW        {name}")
            bad += 1
            continue
        obody, oinfo = old.pop(oname)
        a, b = normalised(oname, obody), normalised(name, body)
        ra, rb = resources(oinfo), resources(info)
        same = a == b and ra == rb
        bad += not same
        print(f"{'identical' if same else 'DIFFERENT'}  {name}" + (f"  (was {oname})" if oname != name else ""))
        print(f"           {len(b)} lines, " + " ".join(f"{k}={v}" for k, v in rb.items()))
        if a != b:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print(f"           first difference at line {i} of {len(a)} / {len(b)}")
        if ra != rb:
            print(f"           was " + " ".join(f"{k}={v}" for k, v in ra.items()))
    for oname in old:
        print(f"removed    {oname}")
    print(f"{len(new)} kernels, {len(new) - bad} identical to their parent, {len(old)} removed")
    return 1 if bad else 0


def main(path, pat=""):
    for name, (body, info) in kernels(path).items():
        if pat not in name:
            continue
        V0 = r"vmcnt\(0\)"

        def cnt(r):
            return len(re.findall(r, body))
        r = resources(info)
        print(f"{name[:90]}\n   vgpr={r['NumVgprs']} agpr={r['NumAgprs']} scratch={r['ScratchSize']} "
              f"occ={r['Occupancy']} mfma={cnt(r'v_mfma')} ds_read={cnt(r'ds_read')} glds={cnt(r'global_load_lds')} "
              f"vmcnt={cnt(r'vmcnt')} vmcnt0={cnt(V0)} barrier={cnt(r's_barrier')} scratch_ops={cnt(r'scratch_')}")


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        sys.exit(diff(*sys.argv[2:]))
    main(*sys.argv[1:])
