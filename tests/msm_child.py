"""Child process of test_msm_gpu.py: loads the profiling build and runs the sums of the two verdict algorithms on the device
under the chosen scalars of tests/msm_cases.py -- one jjs_debug_msm_dev call per (window width, shape, case group): the
buckets' offsets, the sorted entries bucket by bucket as sets, every window sum and the total; one jjs_debug_keyset_sums_dev
call per key-set case: every S_k and the sum of the key points.  Every comparison is an equality of integers or of points
against the Python reference, which worker processes started before the device is opened compute meanwhile.  Prints "ok"
and exits 0 when every check holds."""
import ctypes
import multiprocessing
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import msm_cases as mc  # noqa: E402


def msm_refs(cs):
    return [mc.msm_reference(g, *cs) for g in mc.msm_groups(*cs)]


def keyset_refs(sn):
    return mc.keyset_keys(*sn)[1], mc.keyset_cases(*sn)


def main() -> None:
    t0 = time.time()
    mc.points()
    workers = max(1, min(8, len(os.sched_getaffinity(0)) - 1))
    pool = ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("fork"))      # before this process opens the device
    ks_jobs = [pool.submit(keyset_refs, sn) for sn in mc.KEYSET_SETS]
    jobs = [pool.submit(msm_refs, cs) for cs in sorted(mc.SHAPES, key=lambda cs: -cs[0])]
    jobs = dict(zip(sorted(mc.SHAPES, key=lambda cs: -cs[0]), jobs))

    import torch
    import jubjub_schnorr_amd as jjs
    from jubjub_schnorr_amd import _ffi
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    words = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    host = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

    # the bucket MSM: every width in both shapes
    mc.CLASS_COUNTS.clear()
    calls = 0
    for c, short in mc.SHAPES:
        W, B, _, _ = mc.shape(c, short)
        queued = []
        for g in mc.msm_groups(c, short):
            pts, sc = mc.msm_inputs(g)
            N = len(sc)
            buf = [dev(pts), dev(sc), words(W * B + 1), words(N * W), words(36 * W), words(36)]
            _ffi.check(lib.jjs_debug_msm_dev(ptr(buf[0]), ptr(buf[1]), g["n"], g["n_kinds"], g["neg_kinds"], c, int(short), ptr(buf[2]),
                                             ptr(buf[3]), ptr(buf[4]), ptr(buf[5]), stream()), "jjs_debug_msm_dev")
            queued.append((g, buf))
            calls += 1
        torch.cuda.synchronize()
        for (g, buf), ref in zip(queued, jobs[(c, short)].result()):
            off, order, win, total = (host(t) for t in buf[2:])
            mc.check_msm(ref, off, order[:off[-1]], win.reshape(W, 36), total, (c, short, g["name"]), mc.point_eq_limbs)
            if g["name"] == "scalars":
                mc.check_end_slots(c, short, ref)
                if not short:
                    mc.check_top_slots(c, ref)
        del queued
    mc.assert_msm_classes()
    t1 = time.time()
    print("msm: %d calls over %d (width, shape) pairs, %.1f s" % (calls, len(mc.SHAPES), t1 - t0))

    # the run sums and the key points of the key-set verdict
    calls = 0
    for (scheme, nk), job in zip(mc.KEYSET_SETS, ks_jobs):
        keys, cases = job.result()
        cols = len(keys)
        with eng.keyset(scheme, *keys) as ks:
            assert ks.key_status.tolist() == [int(k == nk // 2) for k in range(nk)]          # the identity key is registered as not valid
            queued = []
            for case in cases:
                buf = [dev(case["idx"])] + [dev(a) for a in case["a"]] + [torch.zeros(cols * nk * 32, dtype=torch.uint8, device="cuda"), words(36)]
                _ffi.check(lib.jjs_debug_keyset_sums_dev(ks.handle, ptr(buf[0]), ptr(buf[1]), ptr(buf[2]) if cols > 1 else None, case["n"],
                                                         ptr(buf[-2]), ptr(buf[-1]), stream()), "jjs_debug_keyset_sums_dev")
                queued.append((case, buf))
                calls += 1
            torch.cuda.synchronize()
            for case, buf in queued:
                mc.check_keyset(case, buf[-2].cpu().numpy().reshape(cols, nk, 32), host(buf[-1]), case["name"], mc.point_eq_limbs)
    pool.shutdown()
    print("key sets: %d calls over %d sets, %.1f s" % (calls, len(mc.KEYSET_SETS), time.time() - t1))
    print("ok")


if __name__ == "__main__":
    main()
