"""Per-phase cycle breakdown of the fused update kernel (diagnostic build with s_memtime
stamps; only the shares are meaningful, the stamps themselves cost a little)."""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from ddrl_amd import build, native as N
extra = os.environ.get("DDRL_EXTRA_FLAGS", "").split()
tag = "".join(ch for ch in "".join(extra) if ch.isalnum())[:24]
# prebuilt (here, on the CPU) when DDRL_STAMPS_LIB names it: python tools/diag_stamps.py --build
# DDRL_STAMPS_LIB=1: libddrl_hip_stamps.so; any other value: that file name in ddrl_amd/ (variants)
_sl = os.environ.get("DDRL_STAMPS_LIB", "1")
stamps_lib = os.path.join(os.path.dirname(N.LIB_PATH), "libddrl_hip_stamps.so" if _sl in ("", "1") else _sl)
if "--build" in sys.argv or not os.environ.get("DDRL_STAMPS_LIB"):
    lib = build.build(extra_flags=["-DDDRL_STAMPS"] + extra,
                      lib=stamps_lib if "--build" in sys.argv else
                      os.path.join(os.path.dirname(N.LIB_PATH), f"libddrl_hip_diag{tag}.so"),
                      build_dir=os.path.join(os.path.dirname(N.LIB_PATH), f"_build_diag{tag}"))
    if "--build" in sys.argv:
        print(lib)
        sys.exit(0)
else:
    lib = stamps_lib
N.load(lib)
from ddrl_amd.spec import make_cfg
from ddrl_amd.trainer import glorot_ffn_flat
n, T = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 512, 200
cfg, inst = make_cfg("QuantrupedMultiEnv_Local", n, T)
ctx = N.Context(cfg, 0, torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(0)
for p in range(4):
    ctx.params_set(p, glorot_ffn_flat(rng, 35, 2))
recs = []
for p in range(4):
    lay = ctx.layout[p]
    r = rng.normal(size=(T * lay["C"], lay["stride"])).astype(np.float32) * 0.5
    r[:, lay["logit"] + 2:lay["logit"] + 4] = -0.5
    ctx.records_set(p, r)
R = T * n; nb = R // 128
sh = [torch.from_numpy(rng.permutation(R).astype(np.int32)).cuda() for _ in range(4)]
pe = [torch.from_numpy(np.stack([rng.permutation(nb) for _ in range(10)]).astype(np.int32)).cuda() for _ in range(4)]
steps = 10 * nb
for it in range(2):
    t0 = time.perf_counter()
    ctx.ppo_update(0xF, sh, pe, [0.2] * 4)
    ctx.synchronize()
    dt = time.perf_counter() - t0
st = (ctypes.c_ulonglong * (32 * 16))()
assert N.load().ddrl_diag_stamps(st) == 0
split = os.environ.get("DDRL_UPDATE_SPLIT", "2") != "1"
blocks = [0, 8, 16] if split else [0, 8]
labels = ["policy rows 0-63", "policy rows 64-127", "value rows 0-63"] if split else ["policy", "value"]
a = np.array(st, dtype=np.float64).reshape(32, 16)[blocks, :15] / steps
# The one-barrier weight-gradient phase (update_dwb, ppo_ffn_impl.h) has neither sync #2 nor the
# store block and sync #3: its X store sits in "fwd" (step head), its dZ1 stores in "layer2 bwd+db1",
# the policy's small-parameter puts in "dW2 tiles (+out)", and the two stamps between are empty.
names = ["fwd", "loss", "dpp head/bias", "head bwd+db2+stores", "layer2 bwd+db1 (+dZ1 stores)", "sync#1 (+gs/stats out)",
         "dW2 tiles (+out)", "sync#2 (two-barrier form)", "X/dZ1 stores + sync#3 (two-barrier form)", "prefetch issue", "dW1 tiles",
         "norm exchange", "adam", "sync#6", "partner exchange (split)"]
print(f"steps {steps}, {dt / steps * 1e6:.2f} us/step wall")
if hasattr(N.load(), "ddrl_diag_poll_stale"):
    # first partner polls that missed, per wave (waves 0 .. 2 issue the record gathers behind the
    # poll's loads; a re-poll queues behind them)
    ps = (ctypes.c_uint * (32 * 8))()
    assert N.load().ddrl_diag_poll_stale(ps) == 0
    ps = np.array(ps, dtype=np.float64).reshape(32, 8)
    for b in range(0, 32, 8):
        print(f"block {b:2d}: first poll stale, waves 0-3: " + " ".join(f"{100 * x / steps:5.1f}%" for x in ps[b, :4]))
fw = None
if hasattr(N.load(), "ddrl_diag_fwd_stamps"):
    # splits of the forward stamp, in time order: layer 1, layer 1 -> layer 2 gap, layer 2, tail
    fs = (ctypes.c_ulonglong * (32 * 4))()
    assert N.load().ddrl_diag_fwd_stamps(fs) == 0
    fw = np.array(fs, dtype=np.float64).reshape(32, 4)[blocks] / steps
for wg in range(len(blocks)):
    tot = a[wg].sum()
    print(f"{labels[wg]} WG: {tot:.0f} cycles/step")
    for k, nm in enumerate(names):
        print(f"   {nm:45s} {a[wg, k]:8.0f}  {100 * a[wg, k] / tot:5.1f}%")
        if k == 0 and fw is not None:
            head = a[wg, 0] - fw[wg].sum()
            for nm2, v in [("step head (alpha, load_row)", head), ("layer 1", fw[wg, 0]), ("layer 1 -> layer 2 gap", fw[wg, 1]),
                           ("layer 2", fw[wg, 2]), ("tail (tanh, head, cup)", fw[wg, 3])]:
                print(f"      fwd: {nm2:38s} {v:8.0f}  {100 * v / tot:5.1f}%")
