"""Backward-pass diagnostics table (does not stop at the first failure): the backward_checks table, then the per-case tolerance ratios of
tests/backward_kernel_checks.py (every dispatch route of the backward, LoRA and optimizer kernels against fp64; ratio <= 1 passes)."""
import os, sys, traceback
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tests import backward_checks as bc
from tests.conftest import GOLDEN
gl = lambda name: torch.load(os.path.join(GOLDEN, name), map_location="cpu", weights_only=True)
for fn in bc.ALL + [lambda: bc.check_model_grads(gl)]:
    try:
        for name, e, t in fn():
            print(f"{'ok  ' if e <= t else 'FAIL'} {name:60s} err {e:.3e} tol {t:.3e}", flush=True)
    except Exception:
        print("EXC in", getattr(fn, "__name__", "model_grads"))
        traceback.print_exc()

from tests import backward_kernel_checks as bk
from tests import test_backward_kernels_gpu as tg
from llmseg_amd import _lib, ops
nbad = 0
for case in bk.cases():
    if case.einval:
        try:
            getattr(tg, "run_" + case.op)(case, bk.reference(case)[0], ops)[0]()
            nbad += 1
            print(f"FAIL {case.name:50s} no error raised")
        except RuntimeError as e:
            ok = case.einval in str(e)
            nbad += not ok
            print(f"{'ok  ' if ok else 'FAIL'} {case.name:50s} refused: {e}")
        continue
    try:
        inp, ref, bounds = bk.reference(case)
        call, outs, guarded = getattr(tg, "run_" + case.op)(case, inp, ops)
        n0 = _lib.load().llmseg_launch_count()
        call()
        launches = _lib.load().llmseg_launch_count() - n0
        torch.cuda.synchronize()
        r = bk.ratios({n: get().cpu() for n, get in outs.items()}, ref, bounds)
        ok = all(x <= 1.0 for x in r.values()) and launches == case.launches and all(g.guard_untouched() for g in guarded)
        nbad += not ok
        print(f"{'ok  ' if ok else 'FAIL'} {case.name:50s} launches {launches} (table {case.launches})  " + " ".join(f"{n}={x:.3f}" for n, x in r.items()), flush=True)
    except Exception as e:
        nbad += 1
        print("EXC in", case.name)
        traceback.print_exc()
        if isinstance(e, RuntimeError) and any(k in str(e) for k in ("HIP", "hip", "CUDA", "device-side", "illegal memory")):
            print("a GPU runtime error: nothing more is started on this device")
            break
print("backward_kernel_checks failures:", nbad)
