"""Did a change move the ISA of kernels it was not meant to touch?  Per-symbol comparison of gfx950 assembly (no GPU needed).

  python3 tools/isa_diff.py A B [--file rtk_trace.hip] [--flags "-DRTK_PROFILE"] [substring ...]

A and B are .s files, or git revisions ("HEAD~1", "HEAD"; "." = the working tree): csrc/<file> of each is compiled to assembly
with the library's own flags (__graft_entry__.hip_build_command).  Comments, the function index inside local labels
(.LBB<n>_k, .Lfunc_end<n>) and the __hip_cuid_<hash> symbol are masked: they follow a function's position in its file and the
file's text, not the code.  Exit status 1 if a symbol present on both sides (and matching a substring, if any) differs.
"""
import argparse, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import hip_build_command  # noqa: E402


def functions(path):
    out, cur, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, buf = m.group(1), []
        if cur is None:
            continue
        ends = ".end_amdhsa_kernel" in line or (line.startswith(".Lfunc_end") and "_kernel" not in cur and "rtk_isa_probe" not in cur)
        line = re.sub(r"__hip_cuid_\w+", "CUID", re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", re.sub(r"BB\d+_", "BB_", line.split(";", 1)[0])))
        if line.split():
            buf.append(" ".join(line.split()))
        if ends:
            out[cur], cur = "\n".join(buf), None
    return out


def assembly(what, name, flags, tmp):
    if what.endswith(".s"):
        return what
    tree = ROOT
    if what != ".":  # a revision: its whole tree, so that the file sees its own headers
        tree = os.path.join(tmp, "tree_" + re.sub(r"\W", "_", what))
        os.makedirs(tree)
        subprocess.check_call("git archive %s | tar -x -C %s" % (what, tree), shell=True, cwd=ROOT)
    out = os.path.join(tmp, re.sub(r"\W", "_", what) + ".s")
    cmd = hip_build_command(out, flags, sources=(name,), mode=("-S", "--cuda-device-only"))
    subprocess.check_call([a.replace(ROOT, tree) if a.startswith(("-I", ROOT)) else a for a in cmd], stderr=subprocess.DEVNULL)
    return out


ap = argparse.ArgumentParser()
ap.add_argument("a"), ap.add_argument("b"), ap.add_argument("want", nargs="*")
ap.add_argument("--file", default="rtk_trace.hip"), ap.add_argument("--flags", default="")
args = ap.parse_args()
with tempfile.TemporaryDirectory() as tmp:
    a, b = (functions(assembly(w, args.file, args.flags.split(), tmp)) for w in (args.a, args.b))
common = sorted(k for k in set(a) & set(b) if not args.want or any(w in k for w in args.want))
bad = [k for k in common if a[k] != b[k]]
print(f"symbols: {len(a)} / {len(b)}; compared {len(common)}; identical {len(common) - len(bad)}")
print(f"rtk_render_kernel: {sum('rtk_render_kernel' in k for k in a)} / {sum('rtk_render_kernel' in k for k in b)}; differing {sum('rtk_render_kernel' in k for k in bad)}")
for tag, names in (("only in first :", set(a) - set(b)), ("only in second:", set(b) - set(a)), ("DIFFERS:", bad)):
    for k in sorted(names):
        print(" ", tag, k[:100])
sys.exit(1 if bad else 0)
