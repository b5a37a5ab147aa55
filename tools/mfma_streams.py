"""Per-kernel figures of the MFMA streams in a translation unit's device assembly.

    python tools/mfma_streams.py [--tree ROOT] [--asm FILE.s] [FILE.hip ...] [-- extra flags]

Each FILE.hip (a name under ddrl_amd/csrc of the tree, default ppo_ffn.hip) is compiled to
assembly with the flags ddrl_amd/build.py gives that file (FLAGS + its SRC_FLAGS entry + the flags
after `--`, plus `--cuda-device-only -S`); `--asm` reads an assembly file instead.  Needs hipcc
only: no GPU, no import of the library.  Printed per kernel:

  insts      instructions
  mfma       v_mfma_* among them
  dep_pairs  MFMAs issued directly behind an MFMA that writes their accumulator (s_nop between
             them ignored): the second waits out the dependent latency (40 cycles against 32 of
             issue for v_mfma_f32_16x16x4_f32)
  bursts     exposed LDS bursts: a run of ds_read / ds_load instructions, then an s_waitcnt with
             lgkmcnt(0), then an MFMA -- the whole LDS round trip lies between two MFMAs
  acc_moves  v_accvgpr_read / v_accvgpr_write / v_accvgpr_mov
  vgpr, agpr, scratch   from the kernel's resource comments (scratch in bytes per lane)
"""
import argparse, importlib.util, os, re, shutil, subprocess, sys

_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_REG = re.compile(r"[av](?:\[\d+:\d+\]|\d+)")
_RES = {"vgpr": re.compile(r";\s*NumVgprs:\s*(\d+)"), "agpr": re.compile(r";\s*NumAgprs:\s*(\d+)"),
        "scratch": re.compile(r";\s*ScratchSize:\s*(\d+)")}


def _insts(lines):
    """(mnemonic, operand text) of every instruction line."""
    out = []
    for l in lines:
        s = l.split(";", 1)[0].strip()
        if not s or s.startswith(".") or _LABEL.match(s):
            continue
        m, _, ops = s.partition(" ")
        out.append((m, ops.strip()))
    return out


def stream_stats(lines):
    """The figures of one kernel's body (a list of assembly lines)."""
    ins = [i for i in _insts(lines)]
    flow = [i for i in ins if i[0] != "s_nop"]   # what issues, padding aside
    st = dict(insts=len(ins), mfma=0, dep_pairs=0, bursts=0, acc_moves=0)
    for k, (m, ops) in enumerate(flow):
        if m.startswith("v_accvgpr_"):
            st["acc_moves"] += 1
        if not m.startswith("v_mfma"):
            continue
        st["mfma"] += 1
        if k == 0:
            continue
        pm, pops = flow[k - 1]
        regs = _REG.findall(ops)
        if pm.startswith("v_mfma"):
            pregs = _REG.findall(pops)
            if pregs and len(regs) >= 2 and regs[-1] == pregs[0]:   # srcC of this one == dst of the last
                st["dep_pairs"] += 1
        elif pm == "s_waitcnt" and "lgkmcnt(0)" in pops and k >= 2 and flow[k - 2][0].startswith(("ds_read", "ds_load")):
            st["bursts"] += 1
    return st


def kernels(text):
    """{kernel name: (body lines, resources)} of an assembly text, in file order."""
    lines = text.splitlines()
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    out = {}
    for name in names:
        try:
            a = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        except StopIteration:
            continue
        b = next((i for i in range(a + 1, len(lines)) if lines[i].lstrip().startswith((".Lfunc_end", ".section", ".amdhsa_kernel"))),
                 len(lines))
        res = {}
        for l in lines[b:b + 80]:   # the resource comments follow the body
            for key, rx in _RES.items():
                m = rx.search(l)
                if m and key not in res:
                    res[key] = int(m.group(1))
        out[name] = (lines[a + 1:b], res)
    return out


def compile_asm(root, name, extra):
    spec = importlib.util.spec_from_file_location("_ddrl_build", os.path.join(root, "ddrl_amd", "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)   # build.py alone: the package (and its native library) is not imported
    cmd = [B.HIPCC, *B.FLAGS, *B.SRC_FLAGS.get(name, []), *extra, "--cuda-device-only", "-S",
           os.path.join(B.CSRC, name), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {name}:\n{r.stderr.decode()[-2000:]}")
    return r.stdout.decode()


def _demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True)
        out = r.stdout.splitlines()
        if len(out) != len(names):
            return names
        # "void ns::k<2, 9>(Args, ...)" -> "k<2, 9>": the template instance is what tells kernels apart
        short = [re.search(r"(\w+(?:<[^()]*>)?)\(", x) for x in out]
        return [m.group(1) if m else x for m, x in zip(short, out)]
    except (OSError, subprocess.CalledProcessError):
        return names


def report(title, text):
    ks = kernels(text)
    print(f"# {title}")
    print(f"{'insts':>7} {'mfma':>5} {'dep_pairs':>9} {'bursts':>6} {'acc_moves':>9} {'vgpr':>5} {'agpr':>5} {'scratch':>7}  kernel")
    for (name, (body, res)), pretty in zip(ks.items(), _demangle(list(ks))):
        st = stream_stats(body)
        print(f"{st['insts']:7d} {st['mfma']:5d} {st['dep_pairs']:9d} {st['bursts']:6d} {st['acc_moves']:9d} "
              f"{res.get('vgpr', -1):5d} {res.get('agpr', -1):5d} {res.get('scratch', -1):7d}  {pretty}")


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    extra = []
    if "--" in argv:
        extra, argv = argv[argv.index("--") + 1:], argv[:argv.index("--")]
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("files", nargs="*", help="translation units under ddrl_amd/csrc (default ppo_ffn.hip)")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--asm", action="append", default=[], help="an assembly file to read instead of compiling")
    a = ap.parse_args(argv)
    for path in a.asm:
        report(path, open(path).read())
    for name in a.files or ([] if a.asm else ["ppo_ffn.hip"]):
        report(name + (" " + " ".join(extra) if extra else ""), compile_asm(a.tree, name, extra))
    return 0


if __name__ == "__main__":
    sys.exit(main())
