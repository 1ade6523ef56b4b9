"""Solver base class: the randomized vector rounding on the device.

Same surface as the reference's `sdp_solver` (sim_src/alg/sdp_solver.py:9-107): constructor
`(nit, rank_radio, alpha)`, `run_with_state`, `rounding(Z, gX, state, nattempt=10)` and
`rounding_one_attempt(Z, gX, state)` returning `(z_vec float64[K], Z, remainder)`.
The projection, the preference ordering and the greedy slot assignment run in HIP kernels
(`mmw_round`, include/mmw_hip.h); the host only draws the `Z x D'` projection vectors and the slots
of users left unassigned from the global NumPy stream, in the reference's order
(sdp_solver.py:48,105), so a seeded run consumes the stream identically.
"""
import numpy as np

from . import _lib
from .stats import STATS_OBJECT


class sdp_solver:
    def __init__(self, nit=100, rank_radio=2, alpha=1.):
        self.nit = nit
        self.rank_radio = rank_radio
        self.alpha = alpha  # objective scaling factor, unused (sdp_solver.py:13)
        self._dev = None  # (state arrays identity, _lib.Solver)

    # ---- device handle keyed by the state's content identity ---------------------------------
    _device_index = 0
    _dtype_code = _lib.F64

    def _state_key(self, state):
        S, Q, h = state
        return (S.shape[0], S.nnz, Q.nnz, float(S.data[:8].sum()) if S.nnz else 0.0, int(S.indices[:8].sum()) if S.nnz else 0,
                float(np.asarray(h)[:8].sum()))

    @staticmethod
    def _state_K(state):
        return state.K if isinstance(state, _lib.DeviceState) else state[0].shape[0]

    def _same_state(self, state):
        """Content comparison with the arrays the handle was created from (copies taken then): in-place edits of
        `S.data` between two calls are seen, like the reference which re-reads the state on every run (mmw.py:28)."""
        if self._dev is None:
            return False
        key, held, _ = self._dev
        if isinstance(state, _lib.DeviceState) or isinstance(held, _lib.DeviceState):
            return held is state  # a device-resident state is immutable: identity is content
        if key != self._state_key(state):
            return False
        S, Q, h = state
        (sp0, si0, sx0), (qp0, qi0), h0 = held
        return np.array_equal(S.indptr, sp0) and np.array_equal(S.indices, si0) and np.array_equal(S.data, sx0) and \
            np.array_equal(Q.indptr, qp0) and np.array_equal(Q.indices, qi0) and np.array_equal(np.asarray(h), h0)

    def _device_solver(self, Z, state, nit=1, eta=None, need_loop=False, warm=False):
        """A device handle holding `state` (reused across the binary search's solve/rounding pairs)."""
        if isinstance(state, _lib.DeviceState):
            state.check()  # (an environment that has moved since: this state's arrays are gone, even where a handle of them is still held)
        if self._same_state(state):
            s = self._dev[2]
            if need_loop:  # same state, another slot count: keep pattern, blocking and device copies
                if eta is not None:
                    s.set_eta(eta)  # the reference reads self.eta on every run
                s.set_slots(max(int(Z), 2), max(int(nit), 1), warm=warm)
            return s
        self.close()
        if isinstance(state, _lib.DeviceState):  # straight from the device (a generator's state or CSR arrays): no host copy of the state at all
            s = state.env.solver(max(int(Z), 2), max(int(nit), 1), 0.1 if eta is None else eta, rank_radio=self.rank_radio,
                                 dtype=self._dtype_code)
            self._dev = (None, state, s)
            return s
        s = _lib.Solver(max(int(Z), 2), state, max(int(nit), 1), 0.1 if eta is None else eta, rank_radio=self.rank_radio,
                        dtype=self._dtype_code, device=self._device_index)
        S, Q, h = state
        held = ((S.indptr.copy(), S.indices.copy(), S.data.copy()), (Q.indptr.copy(), Q.indices.copy()), np.array(h, dtype=np.float64))
        self._dev = (self._state_key(state), held, s)
        return s

    def close(self):
        """Release the device handle (it is also released when the object is collected)."""
        if self._dev is not None:
            self._dev[2].close()
            self._dev = None

    def run_with_state(self, bs_iteration, Z, state):
        pass

    round_batch = False  # True: all attempts of one rounding() call in a single device launch

    round_draws = "host"  # "device" (mmw's keyword): rounding() is one Solver.round_attempts call, the directions drawn on the device
    seed = 0
    _round_calls = 0

    def round_key(self, call):
        """The key of this object's `call`-th rounding() under round_draws="device" (call = 0, 1, ...):
        batch.probe_seed(self.seed, 0, 0x20000 | (call & 0x1FFFF)).  It seeds the device's directions -- attempt a rounds with
        `Solver.round_randv(Z, D', key, a)` -- and the generator that fills the users left over."""
        from .batch import probe_seed
        return probe_seed(self.seed, 0, 0x20000 | (int(call) & 0x1FFFF))

    def _rounding_device(self, Z, gX, state, nattempt):
        """sdp_solver.py:18-25 as ONE device call (`Solver.round_attempts`, key `round_key(n)` for the n-th such call of this
        object): the attempts' directions are drawn on the device, the first attempt that leaves nobody over wins, else the last --
        what the sequential loop over those attempts returns.  The users left over are drawn from `np.random.default_rng(key)`; the
        global NumPy stream is not touched."""
        if not isinstance(gX, _lib.DeviceFactor):
            gX = np.ascontiguousarray(gX, dtype=np.float64)
        key = self.round_key(self._round_calls)
        self._round_calls += 1
        solver = self._device_solver(Z, state)
        z, _, _ = solver.round_attempts(int(Z), gX, max(1, int(nattempt)), key)
        not_assigned = z < 0
        z_vec = z.astype(np.float64)
        if np.any(not_assigned):
            z_vec[not_assigned] = np.random.default_rng(key).integers(0, Z, int(not_assigned.sum()))
        return z_vec, Z, np.sum(not_assigned)

    def rounding(self, Z, gX, state, nattempt=10):
        if self.round_draws == "device":
            return self._rounding_device(Z, gX, state, nattempt)
        if self.round_batch and nattempt > 1:
            return self._rounding_batched(Z, gX, state, nattempt)
        z_vec = None
        remainder = None
        for n in range(nattempt):
            z_vec, Z, remainder = self.rounding_one_attempt(Z, gX, state)
            if remainder == 0:
                return z_vec, Z, remainder
        return z_vec, Z, remainder

    def _rounding_batched(self, Z, gX, state, nattempt):
        """The `nattempt` independent attempts of sdp_solver.py:18-25 as one batch (one workgroup each); the
        first feasible one wins, like the sequential loop.  Draws all projection vectors up front, so the
        global NumPy stream is consumed differently from the reference (use round_batch=False for parity)."""
        if not isinstance(gX, _lib.DeviceFactor):  # (a factor still on the device is read there: no copy out and in again)
            gX = np.ascontiguousarray(gX, dtype=np.float64)
        D = gX.shape[1]
        randv = np.random.randn(nattempt, Z, D)
        randv = randv / np.linalg.norm(randv, axis=2, keepdims=True)
        solver = self._device_solver(Z, state)
        z, rem = solver.round(int(Z), gX, randv)
        ok = np.nonzero(rem == 0)[0]
        pick = int(ok[0]) if ok.size else nattempt - 1
        z = z[pick]
        not_assigned = z < 0
        z_vec = z.astype(np.float64)
        if np.any(not_assigned):
            z_vec[not_assigned] = np.random.randint(Z, size=int(not_assigned.sum()))
        return z_vec, Z, np.sum(not_assigned)

    def rounding_one_attempt(self, Z, gX, state):
        if not isinstance(gX, _lib.DeviceFactor):
            gX = np.ascontiguousarray(gX, dtype=np.float64)
        D = gX.shape[1]
        randv = np.random.randn(Z, D)
        randv = randv / np.linalg.norm(randv, axis=1, keepdims=True)
        solver = self._device_solver(Z, state)
        z, rem = solver.round(int(Z), gX, randv[None])
        z = z[0]
        not_assigned = z < 0
        z_vec = z.astype(np.float64)
        if np.any(not_assigned):
            z_vec[not_assigned] = np.random.randint(Z, size=int(not_assigned.sum()))
        return z_vec, Z, np.sum(not_assigned)


class rand_sdp_solver(sdp_solver):
    """The reference's random embedding (sdp_solver.py:109-114): K x (Z * rank_radio) normals from the global NumPy stream, rows
    normalised, handed to the device rounding above.  The draw is the reference's own expression, so a seeded script continues
    with the same stream.

    Every row of the embedding has norm 1, so the rounding's visiting order (descending norm, sdp_solver.py:51) is one tie over all
    users: sorting the norms as computed sorts their last-bit noise, which changes with the summation order.  `rounding_one_attempt`
    therefore visits the users in index order, the tie rule taken literally (and what the batch does, `BatchSolver.factor_random`):
    it hands the device `index_ordered(gX)`, whose norms fall with the index by steps far above the noise.  Scaling a row by a
    positive number leaves its user's slot preferences as they are.

    draws="device" (opt-in; "host", the default, is everything above, on the same NumPy stream): `run_with_state` draws the embedding
    on the device instead, `Solver.factor_random(Z * rank_radio, key, resident=True, index_order=True)` on the cached handle the
    rounding uses afterwards (built for a `DeviceState` without a host copy of the state), with
    key = batch.probe_seed(seed, 0, 0x40000 | 0) -- `batch.baselines_many`'s key for "rand" at instance 0, so a batch of one and the
    handle agree on the draw.  It returns the block resident and already index-ordered (a `DeviceFactor`), which the rounding
    reads where it lies; the global NumPy stream is not touched by the draw."""

    def __init__(self, nit=100, rank_radio=2, alpha=1., *, draws="host", seed=0, device=0):
        if draws not in ("host", "device"):
            raise ValueError("draws must be 'host' or 'device', got %r" % (draws,))
        sdp_solver.__init__(self, nit=nit, rank_radio=rank_radio, alpha=alpha)
        self.draws = draws
        self.seed = int(seed)  # (0 and device 0 are the base class's own)
        self._device_index = int(device)

    @staticmethod
    def index_ordered(gX):
        if isinstance(gX, _lib.DeviceFactor) and gX.index_ordered:  # scaled on the device already: a second pass would copy it out
            return gX
        K = gX.shape[0]
        return np.asarray(gX, dtype=np.float64) * (1.0 - np.arange(K) * 2.0 ** -32)[:, None]

    def embedding_key(self):
        """The seed of the device's draw: batch.probe_seed(self.seed, 0, 0x40000 | 0)."""
        from .batch import probe_seed
        return probe_seed(self.seed, 0, 0x40000 | 0)

    def rounding_one_attempt(self, Z, gX, state):
        return super().rounding_one_attempt(Z, self.index_ordered(gX), state)

    def _rounding_batched(self, Z, gX, state, nattempt):
        return super()._rounding_batched(Z, self.index_ordered(gX), state, nattempt)

    def _rounding_device(self, Z, gX, state, nattempt):
        return super()._rounding_device(Z, self.index_ordered(gX), state, nattempt)

    draws = "host"

    def run_with_state(self, bs_iteration, Z, state):
        if self.draws == "device":
            solver = self._device_solver(Z, state)
            return True, solver.factor_random(int(Z) * self.rank_radio, self.embedding_key(), resident=True, index_order=True)
        K = self._state_K(state)
        randv = np.random.randn(K, Z * self.rank_radio)
        randv = randv / np.linalg.norm(randv, axis=1, keepdims=True)
        return True, randv


def spectral_laplacian(S_gain):
    """The reference's Laplacian (sdp_solver.py:173-176): D - W of W = S_gain + S_gain^T with the diagonal zeroed, sparse."""
    import scipy.sparse
    import scipy.sparse.csgraph
    W = scipy.sparse.csr_matrix(S_gain + S_gain.transpose())
    W.setdiag(0)
    W.eliminate_zeros()
    return scipy.sparse.csgraph.laplacian(W, normed=False)


class spectral_sdp_solver(STATS_OBJECT, rand_sdp_solver):
    """The reference's spectral embedding (sdp_solver.py:165-185): the Z eigenvectors of largest eigenvalue of the Laplacian of
    S_gain + S_gain^T (diagonal zeroed) as a K x Z block, rows normalised, handed to the shared rounding.  Same positional
    constructor; `run_with_state` logs `spectral_problem_setup` and `spectral_solve` rows [Z, K, microseconds] like the reference.

    K <= 1024 and device >= 0: a batch of one on the device (`BatchSolver.factor_spectral`: a dense Jacobi instead of the reference's
    `eigsh(tol=1e-5)`, eigenvectors to rounding error).  device = -1 or K > 1024: SciPy's `eigsh` on the host, the reference's own
    expression.  Column signs are arbitrary in both.  A user whose row of the block is exactly zero (an isolated user) keeps a zero
    row on the device; the host path divides by zero there, like the reference.

    The rows are unit, so the rounding visits the users in index order through `rand_sdp_solver.index_ordered`, as for the random
    embedding (and as `BatchSolver.round` does on a spectral factor).  A `DeviceState` is read through its host copy.

    handle=True (and device >= 0): a state with K > 1024, and a `DeviceState` of any K, runs on the solver handle instead
    (`Solver.factor_spectral`: the factor's Chebyshev-filtered block iteration on the Laplacian, relative residual 1e-9 against the
    reference's `tol=1e-5`) -- the cached handle the rounding uses afterwards, built for a `DeviceState` without a host copy of the
    state.  `run_with_state` then returns the block resident and already index-ordered (a `DeviceFactor`), which the rounding reads
    where it lies.  Host states with K <= 1024 keep the batch path; handle=False is the behaviour above, unchanged."""

    def __init__(self, nit=100, rank_radio=2, alpha=1., *, device=0, handle=False):
        sdp_solver.__init__(self, nit=nit, rank_radio=rank_radio, alpha=alpha)
        self.device = int(device)
        self.handle = bool(handle)
        if self.device >= 0:
            self._device_index = self.device

    @staticmethod
    def index_ordered(gX):
        if isinstance(gX, _lib.DeviceFactor) and gX.index_ordered:  # scaled on the device already: a second pass would copy it out
            return gX
        return rand_sdp_solver.index_ordered(gX)

    def _run_on_handle(self, bs_iteration, Z, state):
        ps_tic = self._get_tic()
        K = self._state_K(state)
        solver = self._device_solver(Z, state)  # (the Laplacian's values are filled by the handle's first solve, on the device)
        self._add_np_log("spectral_problem_setup", bs_iteration, np.array([Z, K, self._get_tim(ps_tic)]))
        solving_tic = self._get_tic()
        block = solver.factor_spectral(Z, resident=True, index_order=True)
        self._add_np_log("spectral_solve", bs_iteration, np.array([Z, K, self._get_tim(solving_tic)]))
        return True, block

    def run_with_state(self, bs_iteration, Z, state):
        Z = int(Z)
        if self.handle and self.device >= 0 and (isinstance(state, _lib.DeviceState) or self._state_K(state) > _lib.BATCH_EPILOGUE_MAX_K):
            return self._run_on_handle(bs_iteration, Z, state)
        ps_tic = self._get_tic()
        if isinstance(state, _lib.DeviceState):
            state = state.host()
        K = state[0].shape[0]
        on_device = self.device >= 0 and K <= _lib.BATCH_EPILOGUE_MAX_K
        if on_device:
            b = _lib.BatchSolver([2], [state], 1, 0.1, rank_radio=1, device=self.device)  # (its own slot count plays no part: Z goes to the factor)
        else:
            Laplacian = spectral_laplacian(state[0])
        self._add_np_log("spectral_problem_setup", bs_iteration, np.array([Z, K, self._get_tim(ps_tic)]))

        solving_tic = self._get_tic()
        if on_device:
            try:
                b.factor_spectral([Z])
                normed_eigvecs = b.read_factor(0)
            finally:
                b.close()
        else:
            import scipy.sparse.linalg
            _, eigvecs = scipy.sparse.linalg.eigsh(Laplacian, k=Z, which='LM', return_eigenvectors=True, tol=1e-5)
            normed_eigvecs = eigvecs / np.linalg.norm(eigvecs, axis=1, keepdims=True)
        self._add_np_log("spectral_solve", bs_iteration, np.array([Z, K, self._get_tim(solving_tic)]))
        return True, normed_eigvecs
