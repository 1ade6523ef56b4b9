"""Child of tests/test_hip_batch_from_csr.py::test_states_borrowed_from_torch_and_freed: torch touches the device FIRST (a torch build
that ships its own HIP runtime must, before libmmw_hip.so makes its first HIP call in the process), then er120 and golden_env75 go to
the device as sparse-CSR tensors, DeviceCSR.from_torch borrows them and BatchSolver.from_csr builds the batch.  The DeviceCSRs are closed
and the tensors deleted (their memory handed back to the driver) BEFORE the batch completes its host lists and iterates: it reads its
own copy.  Prints `batch from_torch ok` and exits 0 when everything is the host-built batch's."""
import gc
import os
import sys

import numpy as np
import torch

torch.cuda.init()
assert torch.cuda.is_available()
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import csr_cases as cc  # noqa: E402
from sig_sdp_mmw_amd import _lib  # noqa: E402

NAMES = ["er120", "golden_env75"]
NIT, ETA = 3, 0.04
I_LISTS = [getattr(_lib, f) for f in cc.I_FIELDS]
FIELDS = (_lib.F_Y, _lib.F_E_ACCU, _lib.F_E_THIS, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG, _lib.F_XHALF)


def t(m):
    return torch.sparse_csr_tensor(torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int64)), torch.from_numpy(m.data),
                                   size=m.shape, dtype=torch.float64, device=dev)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64)


states = [cc.case(n)[0] for n in NAMES]
Zs = [cc.case(n)[1] for n in NAMES]
tensors = [(t(S), t(Q), torch.from_numpy(np.asarray(h, dtype=np.float64)).to(dev)) for S, Q, h in states]
csrs = [_lib.DeviceCSR.from_torch(*ts) for ts in tensors]
b = _lib.BatchSolver.from_csr(csrs, Zs, NIT, ETA)
for c in csrs:
    c.close()
del tensors, csrs
gc.collect()
torch.cuda.empty_cache()
a = _lib.BatchSolver(Zs, states, NIT, ETA)
assert a.sizes == b.sizes
for i, n in enumerate(NAMES):
    assert [int(v) for v in b.read(i, _lib.BATCH_F_BUILD_INFO)] == [1, 0], n
    for f in I_LISTS + [_lib.I_PATTERN]:
        assert np.array_equal(a.read_i32(i, f), b.read_i32(i, f)), (n, f)
    for f in (_lib.F_S_SUM, _lib.F_NORM_H, _lib.F_ST_DATA, _lib.BATCH_F_PATTERN):
        assert np.array_equal(bits(a.read(i, f)), bits(b.read(i, f))), (n, f)
seeds = np.array([7, 8], dtype=np.uint64)
for x in (a, b):
    x.iterate(NIT, None, seeds)
for i, n in enumerate(NAMES):
    for f in FIELDS:
        assert np.array_equal(bits(a.read(i, f)), bits(b.read(i, f))), (n, f)
a.close(); b.close()
print("batch from_torch ok", flush=True)
