"""Host-side cost of one training step (cProfile) — development aid."""
import cProfile, pstats, sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from egot2_amd import hhi_ttm
from egot2_amd.synth import hhi_args
dev = torch.device("cuda:0")
torch.autograd.set_multithreading_enabled(False)      # the backward's python (EncoderFn.backward) runs in this thread: cProfile sees it


def library_calls(config, steps=200):
    """`python tools/cpu_profile.py --calls c5hhi|c5hoi|c4`: the host time the LIBRARY spends per call in a step of a bench.py workload (the
    C5 steps are launch-bound: their decoder issues ~190 launches) - every egx_* entry point the step calls is timed around its ctypes call."""
    from egot2_amd import _lib, synth
    from egot2_amd import functional as F_egx
    lib = _lib.load()
    wl = synth.make_workload(config, dev, seed=1234)
    spent = {}

    def timed(name, fn):
        def call(*a):
            t = time.perf_counter()
            r = fn(*a)
            rec = spent.setdefault(name, [0, 0.0])
            rec[0] += 1
            rec[1] += time.perf_counter() - t
            return r
        return call

    one = F_egx.unit_grad(dev)

    def step():
        for p in wl["params"]:
            p.grad = None
        wl["loss_fn"]().backward(gradient=one)
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    for name in _lib.SIGNATURES:
        if name.startswith(("egx_encoder_", "egx_decoder_", "egx_translator_")) and not name.endswith("workspace"):
            setattr(lib, name, timed(name, getattr(lib, name)))
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    print(f"{config}: enqueue {1e6 * (t1 - t0) / steps:.0f} us/step over {steps} steps, library {os.environ.get('EGX_LIB', 'product')}")
    for name, (n, s) in sorted(spent.items()):
        print(f"  {name:<28}{n / steps:6.1f} calls/step {1e6 * s / n:8.1f} us/call")


if "--calls" in sys.argv:
    library_calls(sys.argv[sys.argv.index("--calls") + 1])
    sys.exit(0)
m = hhi_ttm.TaskFusionMFTransformer3Task(hhi_args(dropout=0.5)).to(dev).set_compute(sys.argv[1] if len(sys.argv) > 1 else "bf16").train()
feats = [torch.randn(256, 15, 256, device=dev) for _ in range(3)]
target = torch.randint(0, 2, (256,), device=dev)
w = torch.tensor([0.266, 0.734], device=dev)
params = [p for p in m.parameters()]
def step():
    for p in params:
        p.grad = None
    loss = torch.nn.functional.cross_entropy(m.forward_features(*feats), target, weight=w)
    loss.backward()
for _ in range(10):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(200):
    step()
t1 = time.perf_counter()
torch.cuda.synchronize()
t2 = time.perf_counter()
print(f"enqueue {1e6 * (t1 - t0) / 200:.0f} us/step, drained after {1e6 * (t2 - t0) / 200:.0f} us/step")
pr = cProfile.Profile()
pr.enable()
for _ in range(200):
    step()
pr.disable()
torch.cuda.synchronize()
pstats.Stats(pr).sort_stats("cumulative").print_stats(30)
pstats.Stats(pr).sort_stats("tottime").print_stats(30)
