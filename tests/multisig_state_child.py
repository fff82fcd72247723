"""Child process of test_multisig_gpu.py: a fresh engine, so that the multisignature scratch starts unallocated whatever the
parent's tests did before.  Runs multisig_cases.STATE_ORDER on it -- a call that fits the first allocation, one that forces the
scratch to grow and its layout to move, the first call again, then calls in which the transcript beyond the tag table changes
its index -- checks every call against the oracle and every repeated call against its first run, byte for byte, and writes
the outputs to the .npz named on the command line (the parent compares them with the same calls made in another order)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import multisig_cases as mc  # noqa: E402


def main(out_path: str) -> None:
    import torch
    import jubjub_schnorr_amd as jjs
    eng = jjs.engine()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    calls = mc.state_calls(threads=16)
    want = {k: mc.expected(c, threads=16) for k, c in calls.items()}
    first = {}
    for step, name in enumerate(mc.STATE_ORDER):
        a = calls[name].args()
        got = tuple(t.cpu().numpy() for t in eng.multisig_combine(*[dev(x) for x in a[:5]], a[5]))
        mc.check(calls[name], want[name], got, f"step {step} {name}")
        if name in first:
            for k, x, y in zip(mc.OUTPUTS, first[name], got):
                assert (x == y).all(), (step, name, k)
        else:
            first[name] = got
    np.savez(out_path, **{f"{name}.{k}": v for name, got in first.items() for k, v in zip(mc.OUTPUTS, got)})
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
