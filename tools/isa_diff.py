"""Is a change to the kernels' SOURCE a change to their machine code?  Compiles a unit - hijiki_amd/csrc/api/render.hip (the one with
the path kernels) unless --unit names another, by its path from the current directory or from the repository's root - to gfx950
assembly twice - at a git revision and in the working tree - and compares every function's instruction stream (comments and debug
directives dropped; a local label, .LBB<function>_<block>, loses the function's index in the unit, so the order in which the
functions are emitted does not count).  The hygiene work of round 6 (probe hooks instead of #ifdef blocks in the walk, dead build
alternatives removed, one text per shape test) was done under this check: 24 of 24 functions identical.

    python tools/isa_diff.py [REV] [--unit PATH] [--rename REGEX=REPLACEMENT]... [extra hipcc flags]
                                                             # REV defaults to HEAD; exit code 1 when a function differs
REV is the one argument that is neither an option's value nor starts with "-", wherever it stands (so an extra hipcc flag comes in
its joined form: -DNAME=1, -I/path).

Across a rename, functions are matched after every --rename (re.sub, in the order given) has been applied to REV's side: to its
function names and to the symbols its instructions refer to.  A function that exists on one side only after that counts as differing.
"""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-Wno-unused-function", "--cuda-device-only", "-S"]


def functions(path, renames=()):
    text = open(path).read()
    for pat, repl in renames:
        text = re.sub(pat, repl, text)
    out, cur = {}, None
    for l in text.split("\n"):
        m = re.match(r"^(_Z\S+):\s*; @", l)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if l.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is not None:
            t = l.strip()
            if not t or t.startswith(";") or t.startswith(".loc") or t.startswith(".cfi"):
                continue
            out[cur].append(re.sub(r"(\.L[A-Za-z]+)\d+_", r"\1_", re.sub(r";.*$", "", t).rstrip()))
    return out


def compile_tree(root, unit, out, extra, renames=()):
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, "-o", out, os.path.join(root, unit)],
                   check=True, stderr=subprocess.DEVNULL)
    return functions(out, renames)


def main():
    args = sys.argv[1:]
    unit = "hijiki_amd/csrc/api/render.hip"
    if "--unit" in args:
        i = args.index("--unit")
        given = args[i + 1]
        unit = os.path.relpath(os.path.abspath(given if os.path.exists(given) else os.path.join(ROOT, given)), ROOT)
        del args[i:i + 2]
    renames = []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append(tuple(args[i + 1].split("=", 1)))
        del args[i:i + 2]
    revs = [x for x in args if not x.startswith("-")]
    if len(revs) > 1:
        sys.exit(f"isa_diff: one REV at most (got {revs})")
    rev = revs[0] if revs else "HEAD"
    args = [x for x in args if x.startswith("-")]
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(f"git -C {ROOT} archive {rev} hijiki_amd/csrc include | tar -x -C {tmp}", shell=True, check=True)
        old = compile_tree(tmp, unit, os.path.join(tmp, "old.s"), args, renames)
        new = compile_tree(ROOT, unit, os.path.join(tmp, "new.s"), args)
    names = sorted(set(old) | set(new))
    differing = [n for n in names if old.get(n) != new.get(n)]
    for n in names:
        a, b = old.get(n), new.get(n)
        state = "same" if a == b else ("only in " + ("the working tree" if a is None else rev) if a is None or b is None else f"DIFFERS ({len(a)} -> {len(b)} instructions)")
        print(f"{state:40s} {n[:100]}")
    print(f"{len(names)} functions, {len(differing)} differ from {rev}")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
