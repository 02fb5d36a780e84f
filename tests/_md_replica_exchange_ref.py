"""fp64 numpy restatement of anihip_md_exchange (include/anihip.h has the definition): temperature replica exchange between
the entries of a batch, on the Philox4x32-10 and the uniform of tests/_md_ref.py."""
import numpy as np

from _md_ref import KB_HARTREE, MASK, philox4x32_10, uniform  # noqa: F401

EXCHANGE_STEP = 1 << 61


class Ladders:
    """The state of the ladders: slot int32 [L, K] (-1 in the tail of a shorter ladder), rung_kT [L, K] (Hartree, read as the
    fp32 the device holds), C batch entries, ladder_ids [L] or None."""

    def __init__(self, slot, rung_kT, n_entries, ladder_ids=None):
        self.slot = np.array(slot, dtype=np.int32)
        L, K = self.slot.shape
        self.count = (self.slot >= 0).sum(axis=1).astype(np.int32)
        assert ((self.slot >= 0) == (np.arange(K)[None, :] < self.count[:, None])).all(), "the padding must be a tail"
        self.rung_kT = np.asarray(rung_kT, dtype=np.float32).astype(np.float64)
        self.ladder_ids = np.arange(L) if ladder_ids is None else np.asarray(ladder_ids)
        ll, kk = np.nonzero(self.slot >= 0)
        self.rung_of = np.full(n_entries, -1, dtype=np.int32)
        self.ladder_of = np.zeros(n_entries, dtype=np.int32)
        self.rung_of[self.slot[ll, kk]], self.ladder_of[self.slot[ll, kk]] = kk, ll
        self.attempts = np.zeros((L, K - 1), dtype=np.int64)
        self.accepts = np.zeros((L, K - 1), dtype=np.int64)
        self.direction = np.zeros(n_entries, dtype=np.int8)
        self.direction[self.slot[:, 0]] = 1
        self.direction[self.slot[np.arange(L), self.count - 1]] = -1
        self.round_trips = np.zeros(n_entries, dtype=np.int32)
        self.margin = np.inf   # the smallest |ln u - arg| of every decision so far

    def pairs(self, n):
        """(l, k) of every pair of attempt n: k = n (mod 2), k + 1 below the ladder's count."""
        L, K = self.slot.shape
        ll, kk = np.meshgrid(np.arange(L), np.arange(n & 1, K - 1, 2), indexing="ij")
        keep = kk + 1 < self.count[:, None]
        return ll[keep], kk[keep]

    def attempt(self, n, seed, energies, kinetic=None, velocities=None, active=None, wrong_sign=False):
        """Attempt n on energies [C] (Hartree); kinetic [C] and velocities [C, A, 3] (with active [C, A]) are updated in place
        where given.  Returns the number of accepted pairs.  wrong_sign flips the sign of arg: the usual mistake, for the
        test that shows the invariance gate catches it."""
        ll, kk = self.pairs(n)
        a, b = self.slot[ll, kk], self.slot[ll, kk + 1]
        kT_lo, kT_hi = self.rung_kT[ll, kk], self.rung_kT[ll, kk + 1]
        E = np.asarray(energies, dtype=np.float64)
        arg = (1.0 / kT_lo - 1.0 / kT_hi) * (E[a] - E[b])
        if wrong_sign:
            arg = -arg
        step = EXCHANGE_STEP | n
        ctr = np.empty(ll.shape + (4,), dtype=np.uint64)
        ctr[..., 0], ctr[..., 1] = kk, self.ladder_ids[ll].astype(np.uint64) & MASK
        ctr[..., 2], ctr[..., 3] = step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF
        u = uniform(philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64))[..., 0])
        log_u = np.log(u)
        if ll.size:
            self.margin = min(self.margin, float(np.abs(log_u - arg).min()))
        acc = log_u < arg
        self.attempts[ll, kk] += 1
        self.accepts[ll, kk] += acc
        ll, kk, a, b, up = ll[acc], kk[acc], a[acc], b[acc], (kT_hi / kT_lo)[acc]
        down = (kT_lo / kT_hi)[acc]
        self.slot[ll, kk], self.slot[ll, kk + 1] = b, a
        self.rung_of[a], self.rung_of[b] = kk + 1, kk
        if kinetic is not None:
            kinetic[a] *= up
            kinetic[b] *= down
        if velocities is not None:
            act = np.asarray(active)[..., None] != 0
            for e, s in ((a, up), (b, down)):
                scale = np.sqrt(s).astype(np.float32).astype(np.float64)[:, None, None]
                velocities[e] = np.where(act[e], velocities[e] * scale, velocities[e])
        top = kk + 1 == self.count[ll] - 1
        self.direction[a[top]] = -1
        down_to_0 = b[kk == 0]
        self.round_trips[down_to_0] += self.direction[down_to_0] == -1
        self.direction[down_to_0] = 1
        return int(acc.sum())

    def temperatures(self, current, rung_temperatures):
        """``current`` [C] with the ladder members replaced by rung_temperatures [L, K] at their rung."""
        out = np.array(current, copy=True)
        m = self.rung_of >= 0
        out[m] = np.asarray(rung_temperatures)[self.ladder_of[m], self.rung_of[m]]
        return out


def geometric(t_min, t_max, n):
    return t_min * (t_max / t_min) ** (np.arange(n) / (n - 1))


# the invariance case of the CPU and GPU tests: L ladders of K rungs, 300 -> 600 K geometric, every entry's energy drawn from
# Gamma(shape 3) kT of its rung (three harmonic degrees of freedom); (RandomState seed, attempt number) per parity
INVARIANCE_L, INVARIANCE_K, INVARIANCE_SHAPE = 4096, 8, 3.0
INVARIANCE_RUNS = ((5, 0), (6, 1))
INVARIANCE_SEED = (0x1234567 << 32) | 99


def invariance_case(rs_seed):
    """(Ladders with the identity occupancy, energies [L K])."""
    L, K = INVARIANCE_L, INVARIANCE_K
    kT = np.tile((KB_HARTREE * geometric(300.0, 600.0, K)).astype(np.float32), (L, 1))
    lad = Ladders(np.arange(L * K).reshape(L, K), kT, L * K)
    E = np.random.RandomState(rs_seed).gamma(INVARIANCE_SHAPE, 1.0, (L, K)) * lad.rung_kT
    return lad, E.reshape(-1)


def invariance_z(slot, energies, rung_kT):
    """[K]: (per-rung mean of E / (shape kT) - 1) in standard errors 1 / sqrt(shape L), E gathered through ``slot``."""
    L = slot.shape[0]
    ratio = np.asarray(energies)[slot] / (INVARIANCE_SHAPE * rung_kT)
    return (ratio.mean(axis=0) - 1.0) * np.sqrt(INVARIANCE_SHAPE * L)
