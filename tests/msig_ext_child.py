"""Child of test_msig_ext_gpu.py: the affine inline call on the case of `scratch_case()` in a fresh process, whose scratch no
extended call has ever grown; prints the SHA-256 of the five outputs."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def digest(outs) -> str:
    h = hashlib.sha256()
    for a in outs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def scratch_case():
    import multisig_cases as mc
    case = mc.filler(700, seed=77, top=6, threads=16)
    case.bad_z(2, 0, mc.o.R_ORDER)
    return case


if __name__ == "__main__":
    import jubjub_schnorr_amd as jjs
    eng = jjs.engine()
    a = scratch_case().args()
    outs = eng.multisig_combine(*[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a[:5]], a[5])
    torch.cuda.synchronize()
    print("digest", digest([t.cpu().numpy() for t in outs]))
