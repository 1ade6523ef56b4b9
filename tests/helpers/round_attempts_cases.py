"""The scenarios of the one-call rounding tests (mmw_round_attempts, test_round_attempts_host.py, test_hip_round_attempts.py):
moved `online_cases` states, `online_cases.factor`'s recipe at width 2 Z, and a seed whose attempts 0 ... 5 leave the numbers of
users over that make one rule of the choice among attempts visible.  Host-side only: the directions are `philox_ref.randv`, the
attempt is `round_cases.reference_attempt`, and the two rules are restated here on a list of counts."""
import functools

import numpy as np

import online_cases as OC
import philox_ref as pr
import round_cases as RC

NATT = 6
# (case, Z, seed): users left over by attempts 0 ... 5 on the reference's draws, and what the scenario shows
SCENARIOS = {
    ("k75", 9, 0): (0, 1, 1, 1, 1, 0),    # attempt 0 wins
    ("k75", 9, 3): (2, 3, 0, 0, 2, 1),    # the first feasible attempt is 2, not 3
    ("k75", 8, 0): (2, 4, 3, 2, 0, 2),    # feasible only at attempt 4; among the first four: rule 0 takes 3, rule 1 takes 0 (tie with 3)
    ("k192", 9, 3): (2, 3, 5, 4, 1, 3),   # none feasible: rule 0 takes attempt 5, rule 1 attempt 4
}
IDS = ["%s-Z%d-seed%d" % k for k in SCENARIOS]


@functools.lru_cache(maxsize=None)
def factor(name, Z):
    """`online_cases.factor`'s recipe at width 2 Z: unit rows of normals, row k scaled by 1 - k 2^-32 (distinct norms)."""
    K = OC.CASES[name][2]
    g = np.random.default_rng(1000 + K).standard_normal((K, 2 * Z))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    g *= (1.0 - np.arange(K) * 2.0 ** -32)[:, None]
    g.setflags(write=False)
    return g


def pick_of(rem, rule):
    """The attempt a call returns.  rule "first" (sdp_solver.py:18-25): the lowest attempt with nobody left over, else the last;
    "fewest": the fewest left over, ties to the lower attempt."""
    rem = [int(r) for r in rem]
    if rule == "first":
        return rem.index(0) if 0 in rem else len(rem) - 1
    return rem.index(min(rem))


def loop_first(one_attempt, nattempt):
    """The sequential loop with stop-at-first over `one_attempt(a) -> (z, rem)`: returns (z, attempt it ended at)."""
    z = None
    for a in range(nattempt):
        z, rem = one_attempt(a)
        if int(rem) == 0:
            return z, a
    return z, nattempt - 1


@functools.lru_cache(maxsize=None)
def reference_attempts(name, Z, seed, moved=1, nattempt=NATT):
    """(slots int64[nattempt, K], counts) of the reference on its own draws: `philox_ref.randv(Z, 2 Z, seed, a)` through
    `round_cases.reference_attempt` on the case's state."""
    state, gX = OC.host_state(name, moved), factor(name, Z)
    out = [RC.reference_attempt(Z, gX, state, pr.randv(Z, 2 * Z, seed, a))[:2] for a in range(nattempt)]
    return np.stack([z for z, _ in out]), tuple(int(r) for _, r in out)
