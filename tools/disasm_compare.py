"""Do the existing GPU kernels still compile to the same instructions?  Compiles every dclip_amd/csrc/*.hip of a base git
revision and of the working tree device-only (hipcc -O3 --offload-arch=gfx950, the Makefile's flags), disassembles both
with llvm-objdump -d and compares them function by function, with the template arguments stripped from the demangled
names: a kernel that gained a template parameter (the 16-bit type) keeps its name.  Every instruction stream of the base
must appear, unchanged, under the same name in the working tree; functions the working tree adds are listed.  A change that
deletes kernels names them: with --removed NAME[=COUNT] up to COUNT (default: any number of) base functions of that stripped
name may be missing from the working tree; they are listed as removed, not as changed.  Only a fall in the number of
instances of a name counts as a removal: a surviving instance whose code differs is still reported as changed.

    python tools/disasm_compare.py [--base HEAD] [--jobs 8] [--removed NAME[=COUNT] ...]

Exit status 0 when nothing existing changed.  Needs hipcc and git, no GPU."""
from __future__ import annotations

import argparse
import collections
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")
OBJDUMP = os.path.join(ROCM, "llvm", "bin", "llvm-objdump")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-fvisibility=hidden", "-Wno-unused-function",
         "--offload-device-only", "--no-gpu-bundle-output", "-c"]


def strip_templates(name: str) -> str:
    """Demangled name without template arguments (and without the return type a function template prints)."""
    if name.startswith("void "):
        name = name[5:]
    out, depth = [], 0
    for ch in name:
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif depth == 0:
            out.append(ch)
    return "".join(out)


def bare(stripped: str) -> str:
    """The function's own name: no namespaces, no parameter list (what --removed takes)."""
    return stripped.replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]


def functions(code_object: str):
    """{stripped demangled name: [normalised instruction streams]}"""
    txt = subprocess.run([OBJDUMP, "-d", "--demangle", "--no-show-raw-insn", code_object], check=True, capture_output=True,
                         text=True).stdout
    funcs = collections.defaultdict(list)
    name, body = None, []

    def close():
        while body and (body[-1].startswith("s_nop") or body[-1] in ("s_code_end", "...")):    # padding to the next function
            body.pop()
        funcs[strip_templates(name)].append("\n".join(body))

    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            if name is not None:
                close()
            name, body = m.group(1), []
            continue
        if name is None or not line.strip():
            continue
        ins = re.sub(r"//.*$", "", line).strip()        # drop the address / encoding comment
        if ins:
            body.append(re.sub(r"\s+", " ", ins))
    if name is not None:
        close()
    return funcs


def compile_tree(src_root: str, out_dir: str, jobs: int):
    csrc = os.path.join(src_root, "dclip_amd", "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))

    def one(f):
        out = os.path.join(out_dir, f[:-4] + ".co")
        subprocess.run([HIPCC, *FLAGS, os.path.join(csrc, f), "-o", out], check=True, cwd=src_root)
        return f, out

    with cf.ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(one, files))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--base", default="HEAD", help="git revision whose kernels must be unchanged (default HEAD)")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--removed", nargs="*", default=[], metavar="NAME[=COUNT]",
                    help="base functions of this stripped name may be missing from the tree, up to COUNT of them")
    a = ap.parse_args()
    allowance = {}
    for spec in a.removed:
        n, _, c = spec.partition("=")
        allowance[n] = int(c) if c else sys.maxsize
    with tempfile.TemporaryDirectory() as tmp:
        base_src = os.path.join(tmp, "base")
        os.makedirs(base_src)
        arc = subprocess.run(["git", "-C", REPO, "archive", a.base, "dclip_amd/csrc", "include"], check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", base_src], input=arc, check=True)
        os.makedirs(os.path.join(tmp, "b"))
        os.makedirs(os.path.join(tmp, "w"))
        base = compile_tree(base_src, os.path.join(tmp, "b"), a.jobs)
        work = compile_tree(REPO, os.path.join(tmp, "w"), a.jobs)
        changed, same, added, removed = [], 0, [], collections.Counter()
        for f in sorted(set(base) | set(work)):
            fb = functions(base[f]) if f in base else {}
            fw = functions(work[f]) if f in work else {}
            for n, bodies in sorted(fb.items()):
                have = collections.Counter(fw.get(n, []))
                gone = len(bodies) - len(fw.get(n, []))      # a removal lowers the number of instances; what is missing beyond that changed
                for b in bodies:
                    if have[b] > 0:
                        have[b] -= 1
                        same += 1
                    elif gone > 0 and allowance.get(bare(n), 0) > 0:
                        gone -= 1
                        allowance[bare(n)] -= 1
                        removed[f"{f}: {bare(n)}"] += 1
                    else:
                        changed.append(f"{f}: {n}")
            for n, bodies in sorted(fw.items()):
                extra = len(bodies) - len(fb.get(n, []))
                if extra > 0:
                    added.append(f"{f}: {n} (+{extra})")
        print(f"unchanged functions: {same}")
        print(f"added functions: {sum(int(x.rsplit('+', 1)[1][:-1]) for x in added)}")
        for x in added:
            print(f"  + {x}")
        if a.removed:
            print(f"removed functions: {sum(removed.values())}")
            for x, c in sorted(removed.items()):
                print(f"  - {x} (-{c})")
        print(f"changed functions: {len(changed)}")
        for x in changed:
            print(f"  ! {x}")
        return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
