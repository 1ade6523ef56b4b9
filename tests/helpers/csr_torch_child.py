"""Child of tests/test_hip_csr_device.py::test_state_borrowed_from_torch: torch touches the device FIRST (a torch build that ships its own
HIP runtime must, before libmmw_hip.so makes its first HIP call in the process), then er120 goes to the device as sparse-CSR tensors and
DeviceCSR.from_torch borrows them.  Prints `from_torch ok` and exits 0 when the handle is the host-built one."""
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

state, Z = cc.case("er120")
S, Q, h = state


def t(m):
    return torch.sparse_csr_tensor(torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int64)), torch.from_numpy(m.data),
                                   size=m.shape, dtype=torch.float64, device=dev)


tS, tQ, th = t(S), t(Q), torch.from_numpy(np.asarray(h, dtype=np.float64)).to(dev)
try:  # torch's own index arrays are int64: refused, not converted silently
    _lib.DeviceCSR.wrap(tS.crow_indices(), tS.col_indices(), tS.values(), tQ.crow_indices(), tQ.col_indices(), tQ.values(), th, K=S.shape[0])
    raise SystemExit("wrap took int64 index arrays")
except _lib.MMWError as e:
    assert "int64" in str(e), str(e)
c = _lib.DeviceCSR.from_torch(tS, tQ, th)
assert (c.K, c.nnzS, c.nnzQ) == (S.shape[0], S.nnz, Q.nnz)
a = _lib.Solver(Z, state, 3, 0.04)
b = _lib.Solver.from_csr(c, Z, 3, 0.04)
cc.assert_same_handle(a, b, Z)
a.close(); b.close(); c.close()
print("from_torch ok", flush=True)
