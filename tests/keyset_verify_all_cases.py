"""Batches for the tests of jjs_keyset_verify_all* (test_keyset_verify_all_gpu.py, keyset_verify_all_child.py): a batch's
keys registered as a set, its signature columns in each format, and the pair of bad items under one key."""
import numpy as np

import jjs_oracle as o
from helpers import ext_on_device, fe_bytes, make_batch, to_int

KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
RCOLS = {"single": ["R"], "double": ["R", "Rp"], "vargen": ["R"]}


def register_cols(scheme, b):
    """The distinct keys of a batch (the key columns side by side) and each item's index among them."""
    cat = np.ascontiguousarray(np.concatenate([b[k] for k in KEYCOLS[scheme]], 1))
    uniq, inv = np.unique(cat, axis=0, return_inverse=True)
    return [np.ascontiguousarray(uniq[:, 64 * i:64 * i + 64]) for i in range(len(KEYCOLS[scheme]))], inv.reshape(-1).astype(np.uint32)


def compress(points):
    return np.stack([np.frombuffer(o.compress((to_int(r[:32]), to_int(r[32:]))), np.uint8) for r in points])


def sig_cols(eng, scheme, b, fmt):
    """The signature columns and the messages of batch dict b in format fmt (host arrays)."""
    if fmt == "affine":
        return [b["u"]] + [b[k] for k in RCOLS[scheme]] + [b["m"]]
    if fmt == "ext":
        return [b["u"]] + [ext_on_device(eng, b[k]) for k in RCOLS[scheme]] + [b["m"]]
    return [np.ascontiguousarray(np.concatenate([b["u"]] + [compress(b[k]) for k in RCOLS[scheme]], 1)), b["m"]]


def same_key_pair(scheme):
    """Six valid items under ONE key, items 0 and 1 with u_0 + d and u_1 - d: D_0 = -D_1 != O, and both defects meet in the
    same S_k (for the per-item generator the key carries the generator, so d * Gen cancels as well)."""
    b = make_batch(scheme, 6, seed=34, n_keys=1, mix=False)
    d = 12345
    b["u"][0] = fe_bytes((to_int(b["u"][0]) + d) % o.R_ORDER)
    b["u"][1] = fe_bytes((to_int(b["u"][1]) - d) % o.R_ORDER)
    return b
