"""Device assembly of every ddrl_amd/csrc/*.hip of a source tree, and a byte comparison of two trees'.

    python tools/asm_diff.py [--out DIR] [--only GLOB] TREE [TREE2] [-- -DDDRL_XCHG_ATOMIC ...]

Each file is compiled with its tree's build.FLAGS + build.SRC_FLAGS + the flags after `--`, plus
`--cuda-device-only -S`, into DIR/<tree index>/<file>.s with the lines naming the per-compilation
`__hip_cuid_<hash>` symbol dropped.  With two trees: `identical` or the first differing line per
file, exit status 1 on any difference.  A refactor that folds preprocessor switches to their
defaults must leave every file identical.  Needs hipcc only: no GPU, no import of the library.
"""
import argparse, fnmatch, glob, importlib.util, os, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor


def compile_tree(root, extra, out, only):
    spec = importlib.util.spec_from_file_location("_ddrl_build", os.path.join(root, "ddrl_amd", "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)   # build.py alone: the package (and its native library) is not imported
    srcs = [s for s in sorted(glob.glob(os.path.join(B.CSRC, "*.hip"))) if fnmatch.fnmatch(os.path.basename(s), only)]
    os.makedirs(out, exist_ok=True)

    def one(src):
        name = os.path.basename(src)
        cmd = [B.HIPCC, *B.FLAGS, *B.SRC_FLAGS.get(name, []), *extra, "--cuda-device-only", "-S", src, "-o", "-"]
        r = subprocess.run(cmd, capture_output=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr.decode()[-2000:]}")
        with open(os.path.join(out, name + ".s"), "wb") as f:
            f.writelines(l for l in r.stdout.splitlines(keepends=True) if b"__hip_cuid_" not in l)
        return name

    with ThreadPoolExecutor(max_workers=max(1, min(len(srcs), 8))) as ex:
        return list(ex.map(one, srcs))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    extra = []
    if "--" in argv:
        extra, argv = argv[argv.index("--") + 1:], argv[:argv.index("--")]
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("trees", nargs="+", help="one source tree root (compile only) or two (compare)")
    ap.add_argument("--out", help="output directory (default: a new temporary one)")
    ap.add_argument("--only", default="*", help="file name pattern, e.g. 'ppo_ffn*.hip'")
    a = ap.parse_args(argv)
    if len(a.trees) > 2:
        ap.error("at most two trees")
    out = a.out or tempfile.mkdtemp(prefix="asm_diff_")
    names = [compile_tree(t, extra, os.path.join(out, str(i)), a.only) for i, t in enumerate(a.trees)]
    print(f"assembly in {out}")
    if len(a.trees) < 2:
        return 0
    bad = 0
    for name in sorted(set(names[0]) | set(names[1])):
        if name not in names[0] or name not in names[1]:
            print(f"{name}: only in tree {0 if name in names[0] else 1}")
            bad = 1
            continue
        x, y = (open(os.path.join(out, str(i), name + ".s"), "rb").read() for i in (0, 1))
        if x == y:
            print(f"{name}: identical")
            continue
        bad = 1
        lx, ly = x.splitlines(), y.splitlines()
        n = next((k for k, (p, q) in enumerate(zip(lx, ly)) if p != q), min(len(lx), len(ly)))
        a, b = (l[n].decode(errors="replace") if n < len(l) else "<end of file>" for l in (lx, ly))
        print(f"{name}: differs at line {n + 1}:\n  < {a}\n  > {b}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
