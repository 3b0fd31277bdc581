#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds object by object: the kernel symbols and every kernel's instruction list
(__graft_entry__._isa_functions of disassemble_device_code) and the VGPR / AGPR / SGPR / LDS / spill / scratch lines of tools/kernel_resources.py,
compared as sets.  Prints one line per object in the format of profiles/host_launcher_refactor_isa.txt; exit status 1 if anything differs.

    python tools/compare_device_code.py PARENT_BUILD_DIR [NEW_BUILD_DIR]     (directories of *.o; the new one defaults to csrc/build)
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def resources(obj):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), obj], check=True, capture_output=True, text=True)
    return set(r.stdout.splitlines())


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ge.BUILD
    objs = sorted(set(f for d in (old_dir, new_dir) for f in os.listdir(d) if f.endswith(".o")), key=lambda f: (f.endswith("_diag.o"), f))
    total, differ = 0, []
    for o in objs:
        name = o[:-2].replace("_diag", "") + ".hip" + (" (-DCT_DIAG)" if o.endswith("_diag.o") else "")
        a, b = os.path.join(old_dir, o), os.path.join(new_dir, o)
        if not (os.path.exists(a) and os.path.exists(b)):
            differ.append(name)
            print(f"{name}: only in {'the parent' if os.path.exists(a) else 'the new tree'}")
            continue
        try:
            fa, fb = (ge._isa_functions(ge.disassemble_device_code(p), "") for p in (a, b))
        except RuntimeError:  # no gfx950 code object in the file
            print(f"{name}: no kernel")
            continue
        ra, rb = resources(a), resources(b)
        changed = sorted(k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k))
        total += len(fb)
        if changed or ra != rb:
            differ.append(name)
        print(f"{name}: {len(fb)} kernels (parent {len(fa)}); " + (f"{len(changed)} DIFFER in instructions" if changed else "instructions identical") + "; " +
              (f"VGPR / SGPR / LDS / scratch figures identical ({len(rb)} resource lines)" if ra == rb else f"{len(ra ^ rb)} resource lines DIFFER"))
        for k in changed[:8]:
            print(f"    {k}: {len(fa.get(k, []))} -> {len(fb.get(k, []))} instructions")
    print(f"\ntotal: {total} kernels in {len(objs)} objects, " + ("all identical" if not differ else "DIFFERENT: " + ", ".join(differ)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
