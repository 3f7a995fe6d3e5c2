# Measurement aid (GPU box): what the workgroups of the hosted score backward (score_bwd_tr_kernel<4, 2, UNIT, false, true>) do
# behind their sweep, inside the replayed configs[1] step.  Needs a library built with TT_EXTRA_HIPCC_FLAGS=-DTT_POST_STAMPS (the
# stamps are compiled out of the shipped library).  Stamps are thread 0's: a phase that ends at a barrier includes the wait for the
# workgroup's slowest wave.  The clock ticks at 100 MHz: a single phase of a single workgroup reads in steps of 0.01 us.
#     python tools/post_sweep_stamps.py [steps]
import ctypes, sys
sys.path.insert(0, ".")
import numpy as np
import torch
import bench
from jodalrob_twotower_amd import _lib

NAMES = {1: "sweep (thread 0's wave)", 2: "the head's loads issued", 3: "round one written, barrier", 4: "waves 0-3 add and write back, barrier",
         5: "flat sums, dA stored", 6: "barrier: slabs read", 8: "head: Wn, d_y, act^T staged, barrier", 9: "head: column sums, two MFMA chains, barrier",
         10: "head: accumulator -> LDS, barrier", 11: "head: d_act out, da / xhat staged, barrier", 12: "head: ordered S1 / S2, barrier",
         13: "head: partial sums -> LDS, barrier", 14: "head: slabs and partials stored"}


def table(s):
    order = [0] + sorted(NAMES)
    live = (s[:, order] > 0).all(axis=1)
    s = s[live]
    t0 = s[:, 0].min()
    print(f"{int(live.sum())} stamped workgroups; launch span {(s[:, 14].max() - t0) / 100:.2f} us; "
          f"behind the sweep (stamp 1 -> 14): mean {((s[:, 14] - s[:, 1]) / 100).mean():.2f} us, max {((s[:, 14] - s[:, 1]) / 100).max():.2f} us")
    prev = 0
    for i in order[1:]:
        d = (s[:, i] - s[:, prev]) / 100.0
        print(f"  {i:2d} {NAMES[i]:48s} mean {d.mean():6.2f}  p90 {np.percentile(d, 90):6.2f}  max {d.max():6.2f} us")
        prev = i
    st = (s[:, 0] - t0) / 100.0
    print(f"  workgroup start: mean {st.mean():.2f} p90 {np.percentile(st, 90):.2f} max {st.max():.2f} us")


if __name__ == "__main__":
    steps = sys.argv[1] if len(sys.argv) > 1 else "30"
    args = bench.parse(["--no-cpu-baseline", "--no-h2d", "--steps", steps, "--warmup", "10", "--no-lookup-profile", "--no-extra-legs"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = dict(dev=dev, world=1, rank=0, staged=False, comm=None, fence=torch.cuda.synchronize, max_over_ranks=lambda x: x)
    leg = bench.Leg(args, ctx, 8192, 1_000_000, 1_000_000, False)
    leg.run()
    torch.cuda.synchronize()
    fn = _lib.load().tt_debug_post_stamps
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p]
    buf = np.zeros(512 * 16, dtype=np.uint64)
    assert fn(buf.ctypes.data) == 0
    table(buf.reshape(512, 16).astype(np.int64))
    leg.close()
