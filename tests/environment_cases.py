"""The case table of the environment tests and their reference: a longdouble / complex-longdouble einsum walk over host tensors.

E[p, a, s] after `count` tensors, with the conventions of inner(phi, W, psi): the bra is conj(phi) and contracts the operator's
s_out, the ket psi contracts s_in; without an operator a has extent 1.  Left walk: tensors 1 .. count, open legs to their right;
right walk: the last `count` tensors, open legs to their left.  Amplitudes are not applied.

Every case has 5 tensors (the paired one 6: three sites of two).  State bonds come from {1, 2, 3, 5, 16, 17}: 16 | 17 is the edge
of the one-workgroup route; operator bonds from {1, 2, 3, CAP, CAP + 1}.  A walk that does not pass a bond above the cap is
eligible for that route even when the chain has such a bond elsewhere, so the profiles with 17 (CAP + 1) mix the routes over
(side, count)."""
import itertools

import numpy as np

from helpers import random_mpo_data, random_mps_data

CAP = 8                       # QIL_ENV_CHAIN_MAX_OP_BOND
STATE_CAP = 16
EPS = float(np.finfo(np.float64).eps)

# name -> (phi bonds, psi bonds, operator bonds, paired)
CASES = {
    "ones": ((1, 1, 1, 1), (1, 1, 1, 1), (1, 1, 1, 1), False),
    "small": ((2, 3, 5, 3), (1, 2, 3, 2), (1, 2, 3, 2), False),
    "cap": ((2, 16, 16, 2), (2, 5, 16, 3), (2, CAP, CAP, 2), False),
    "over_state": ((2, 17, 16, 2), (2, 16, 17, 2), (2, 3, 2, 2), False),
    "over_op": ((2, 3, 5, 2), (2, 5, 3, 2), (2, CAP + 1, CAP, 2), False),
    "paired": ((2, 3, 4, 3, 2), (2, 4, 5, 4, 2), (2, 3, 2, 3, 2), True),
}
SIDES = ("left", "right")
STATE_MIXES = list(itertools.product((False, True), repeat=2))                # (phi complex, psi complex)
OP_MIXES = list(itertools.product((False, True), repeat=3))                   # (phi, W, psi)


def ntensors(case):
    return len(CASES[case][0]) + 1


def counts(case):
    n = ntensors(case)
    return (0, 1, 2, n - 1, n)


_DATA = {}


def case_data(case, which, complex_):
    """Host tensors of one operand ("phi", "psi", "W") of a case: seeded, computed once, never modified."""
    key = (case, which, bool(complex_))
    if key not in _DATA:
        idx = ("phi", "psi", "W").index(which)
        rng = np.random.default_rng(9100 + 16 * sorted(CASES).index(case) + 2 * idx + int(complex_))
        dt = np.complex128 if complex_ else np.float64
        bonds = CASES[case][idx]
        _DATA[key] = random_mpo_data(bonds, rng, dtype=dt) if which == "W" else random_mps_data(bonds, rng, dtype=dt, normalize=False)
    return _DATA[key]


def _wide(t):
    return np.asarray(t).astype(np.clongdouble if np.iscomplexobj(t) else np.longdouble)


def _identity_site():
    W = np.zeros((1, 2, 2, 1))
    W[0, 0, 0, 0] = W[0, 1, 1, 0] = 1.0
    return W


def reference_environments(phi, W, psi, side):
    """[(E, E_abs, L)] for count = 0 .. n: E the environment in (complex) longdouble, E_abs the same contraction of the |tensors|,
    L the sum over the walked sites of the inner lengths of the three products (s + 2 D + 2 p of the bonds the walk enters a site
    by; s + 2 p without an operator)."""
    n = len(psi)
    order = range(n) if side == "left" else range(n - 1, -1, -1)
    spec = "pas,pyq,axyb,sxt->qbt" if side == "left" else "qbt,pyq,axyb,sxt->pas"
    E = np.ones((1, 1, 1), dtype=np.longdouble)
    Ea = E.copy()
    out, Lsum = [(E, Ea, 0)], 0
    for i in order:
        P, A = _wide(phi[i]), _wide(psi[i])
        Wi = _wide(W[i] if W is not None else _identity_site())
        enter = 0 if side == "left" else -1
        Lsum += A.shape[enter] + 2 * P.shape[enter] + (2 * Wi.shape[enter] if W is not None else 0)
        E = np.einsum(spec, E, P.conj(), Wi, A)
        Ea = np.einsum(spec, Ea, np.abs(P), np.abs(Wi), np.abs(A))
        out.append((E, Ea, Lsum))
    return out


_REF = {}


def reference(case, mix, with_op, side):
    """reference_environments of a case, computed once per (case, dtype mix, operator or not, side)"""
    key = (case, tuple(mix), bool(with_op), side)
    if key not in _REF:
        if with_op:
            pc, wc, sc = mix
            W = case_data(case, "W", wc)
        else:
            (pc, sc), W = mix, None
        _REF[key] = reference_environments(case_data(case, "phi", pc), W, case_data(case, "psi", sc), side)
    return _REF[key]


def bond_dims(case):
    """the n + 1 bond dimensions, edges included, of (phi, psi, W)"""
    return tuple([1] + list(b) + [1] for b in CASES[case][:3])


def chain_eligible(case, with_op, side, count):
    """whether the walked span stays inside the one-workgroup route's caps"""
    n = ntensors(case)
    pd, sd, od = bond_dims(case)
    lo, hi = (0, count) if side == "left" else (n - count, n)
    ok = max(pd[lo:hi + 1]) <= STATE_CAP and max(sd[lo:hi + 1]) <= STATE_CAP
    return ok and (not with_op or max(od[lo:hi + 1]) <= CAP)
