"""Thin object wrapper over the stateful C ABI (``kmc_sampler_*`` in ``include/kissmcmc_hip.h``).

The ensemble lives in HBM for the lifetime of the object; ``run`` enqueues generations of the
reference's ``_emcee`` loop (``src/samplers.jl:245-290``) as HIP kernel launches.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .densities import DeviceLogPdf
from .moves import apply_move
from .tempering import apply_adapt, apply_tempering, thermodynamic_integration


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Sampler:
    def __init__(self, pdf: DeviceLogPdf, nwalkers: int, ndim: int, ngenerations: int, nburnin: int = 0,
                 nthin: int = 1, a_scale: float = 2.0, seed: int = 0, store_chain: bool = False,
                 store_logp: bool = False, moments: bool = False, use_graph: bool = True,
                 device: int = 0, shard_rank: int = 0, shard_count: int = 1, p2p: bool = False,
                 island_gens: int = 0, island_size: int = 0, p2p_finegrained: bool = False, p2p_push: bool = False,
                 dtype: str = "f64", deal_rank: int = 0, deal_count: int = 0,
                 stream_chain: bool = False, chain_by_walker: bool = False, store_blobs: bool = False, move=None,
                 betas=None, ntemps=None, beta_min=None, swap_every: int = 1, temper=None, adapt=None):
        if not isinstance(pdf, DeviceLogPdf):
            raise TypeError(
                "pdf must be a menu log-density (GaussianIso, Exponential, Rosenbrock, LogNormal, MvNormal2), "
                "an ExprDensity (compiled for the device) or a HostLogPdf (any callable, evaluated on the host "
                f"per half-step); got {type(pdf).__name__}.")
        pdf.check_ndim(int(ndim))
        self.pdf = pdf
        self._h = None
        cfg = _lib.Config()
        if dtype not in ("f64", "f32"):
            raise ValueError("dtype must be 'f64' (the reference's Float64) or 'f32' (float rows on the device)")
        cfg.dtype = _lib.F32 if dtype == "f32" else _lib.F64
        cfg.density = pdf.density_id
        p = list(pdf.params()) + [0.0] * 8
        for i in range(8):
            cfg.params[i] = float(p[i])
        cfg.nwalkers, cfg.ndim = int(nwalkers), int(ndim)
        cfg.ngenerations, cfg.nburnin, cfg.nthin = int(ngenerations), int(nburnin), int(nthin)
        cfg.a_scale = float(a_scale)
        cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        flags = 0
        if store_chain:
            flags |= _lib.STORE_CHAIN
        if store_logp:
            flags |= _lib.STORE_LOGP
        if moments:
            flags |= _lib.MOMENTS
        if not use_graph:
            flags |= _lib.NO_GRAPH
        if store_blobs:
            flags |= _lib.STORE_BLOBS      # a CDensity(..., nblob=m): keep the blob of every stored sample (src/samplers.jl:270)
        self.nblob = int(getattr(pdf, "nblob", 0) or 0)
        if stream_chain and (store_chain or store_logp):
            # KMC_STREAM_CHAIN: the chain goes to host arrays block by block while sampling (bounded by host RAM, not HBM)
            flags |= _lib.STREAM_CHAIN
            if chain_by_walker:
                # ... in the reference's order, thetas[w][k]: host arrays [nlocal, nsamples, ndim] / [nlocal, nsamples]
                flags |= _lib.CHAIN_BY_WALKER
        if p2p:
            flags |= _lib.P2P
            if p2p_finegrained:
                flags |= _lib.P2P_FINEGRAINED
            if p2p_push:
                flags |= _lib.P2P_PUSH
        if island_gens:
            # ISLAND MODE: 256-walker islands resident in LDS for `island_gens` generations per launch
            flags |= _lib.ISLANDS
            cfg.island_gens = int(island_gens)
            cfg.island_size = int(island_size)
        cfg.flags = flags
        cfg.device = int(device)
        cfg.shard_rank, cfg.shard_count = int(shard_rank), int(shard_count)
        cfg.deal_rank, cfg.deal_count = int(deal_rank), int(deal_count)   # dealt sub-ensembles (distributed.DealtEmcee)
        apply_move(move, cfg)                  # None: the stretch move; DEMove, DESnookerMove or a weighted list of them (opt-in)
        self.move = move
        # parallel tempering (opt-in): betas=[1, ...], or ntemps= and beta_min= for geometric_betas(ntemps, beta_min); every read-out
        # below stays rung 0's, the rung_* methods return the whole ladder
        # temper="likelihood" (a DataDensity): rung t samples prior + betas[t] * S, the last beta may be 0; rung_loglike*, log_evidence
        # adapt=True or dict(lag=, time=, until=): the sweeps of burn-in move the interior rungs towards equal swap acceptance (README
        # "Adaptive ladder"); `betas` is then the current ladder, `betas0` the one given here
        self.betas0 = apply_tempering(cfg, betas, ntemps, beta_min, swap_every, temper)
        self.adapt = apply_adapt(cfg, adapt)
        self.temper = "likelihood" if cfg.temper_mode == _lib.TEMPER_LIKELIHOOD else ("whole" if self.betas0 is not None else None)
        self.ntemps = 1 if self.betas0 is None else int(self.betas0.size)
        cfg.user_density = pdf.user_handle     # runtime-compiled density (ExprDensity) or None
        cb = getattr(pdf, "c_callback", None)  # host-evaluated density (HostLogPdf) or None
        if cb is not None:
            cfg.host_logpdf = C.cast(cb, C.c_void_p)
            if getattr(pdf, "c_accepted", None) is not None:   # accept outcomes back to the host (blobs)
                cfg.host_accepted = C.cast(pdf.c_accepted, C.c_void_p)
        self.cfg = cfg
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.kmc_sampler_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.nwalkers, self.ndim = int(nwalkers), int(ndim)
        self.nlocal = self.nwalkers // max(1, int(shard_count))
        self.p2p = bool(p2p)
        # rows this object holds: the whole ensemble, or (P2P) this shard's slices of both halves
        self.nrows = self.nlocal if self.p2p else self.nwalkers
        self._host_chain = self._host_logp = None
        self._host_by_walker = False
        if flags & _lib.STREAM_CHAIN and self.nsamples > 0:
            # the destination of the streamed chain: host arrays owned by this object (page-locked in place by the library)
            self._host_by_walker = bool(flags & _lib.CHAIN_BY_WALKER)
            if self._host_by_walker:
                self._host_chain = np.empty((self.nlocal, self.nsamples, self.ndim)) if store_chain else None
                self._host_logp = np.empty((self.nlocal, self.nsamples)) if store_logp else None
            else:
                self._host_chain = np.empty((self.nsamples, self.nlocal, self.ndim)) if store_chain else None
                self._host_logp = np.empty((self.nsamples, self.nlocal)) if store_logp else None
            _lib.check(self._L.kmc_sampler_set_chain_host(self._h, _dp(self._host_chain) if store_chain else None,
                                                          _dp(self._host_logp) if store_logp else None))

    # -- lifecycle --------------------------------------------------------------------------
    def close(self):
        if self._h is not None:
            self._L.kmc_sampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- control ----------------------------------------------------------------------------
    def set_stream(self, hip_stream: int):
        _lib.check(self._L.kmc_sampler_set_stream(self._h, C.c_void_p(hip_stream)))

    def bind_positions(self, device_ptr: int):
        """Use a caller-owned device buffer (``double [nwalkers][ndim]``) for the ensemble."""
        _lib.check(self._L.kmc_sampler_bind_positions(self._h, C.c_void_p(device_ptr)))

    @staticmethod
    def p2p_connect_local(shards):
        """Wire KMC_P2P samplers that live in this process (``shards[r]`` = shard r, same device) to each other."""
        arr = (C.c_void_p * len(shards))(*[s._h for s in shards])
        for s in shards:
            _lib.check(s._L.kmc_sampler_p2p_connect_local(s._h, arr))

    def p2p_link_probe(self, peer: int, nrows: int, reps: int = 20):
        """(GB/s of whole rows of shard ``peer`` gathered at random row indices with the pull's system-scope loads, GB/s of the runtime's
        copy of that shard): one fabric link -- or local memory for ``peer`` = own rank -- measured; the peers must be idle."""
        g, c = C.c_double(0.0), C.c_double(0.0)
        _lib.check(self._L.kmc_sampler_p2p_link_probe(self._h, int(peer), int(nrows), int(reps), C.byref(g), C.byref(c)))
        return g.value, c.value

    @staticmethod
    def rccl_unique_id() -> bytes:
        """A fresh RCCL unique id (rank 0 creates it; every rank of the communicator gets the same bytes)."""
        buf = C.create_string_buffer(_lib.RCCL_ID_BYTES)
        _lib.check(_lib.lib().kmc_rccl_unique_id(buf))
        return buf.raw

    def rccl_init(self, unique_id: bytes):
        """Replica sharding (``shard_rank / shard_count``, no P2P): attach an RCCL communicator; :meth:`run` then enqueues an
        in-place all-gather of the updated half after every half-step kernel.  Collective over all ``shard_count`` ranks."""
        assert len(unique_id) == _lib.RCCL_ID_BYTES
        buf = C.create_string_buffer(bytes(unique_id), _lib.RCCL_ID_BYTES)
        _lib.check(self._L.kmc_sampler_rccl_init(self._h, buf))

    def rccl_capture(self) -> bool:
        """Capture the chunk of kernels + all-gathers now; whether THIS rank got a graph (reduce over the ranks with MIN,
        then :meth:`rccl_set_capture` on every rank: all replay captured all-gathers, or all enqueue them one by one)."""
        got = C.c_int(0)
        _lib.check(self._L.kmc_sampler_rccl_capture(self._h, C.byref(got)))
        return bool(got.value)

    def rccl_set_capture(self, use_captured: bool):
        _lib.check(self._L.kmc_sampler_rccl_set_capture(self._h, 1 if use_captured else 0))

    @staticmethod
    def rccl_version():
        """``"major.minor.patch"`` of the librccl.so the library resolves (``None`` when it cannot be loaded); no device needed."""
        v = C.c_int(0)
        if _lib.lib().kmc_rccl_version(C.byref(v), None, 0) != _lib.OK:
            return None
        return f"{v.value // 10000}.{v.value // 100 % 100}.{v.value % 100}"

    LAUNCH_MODES = {0: "undecided", 1: "table graph", 2: "eager", 3: "updated graph", 4: "single launch per many generations"}

    def launch_mode(self):
        """``(mode, budget_fallback)``: how :meth:`run` issues the launches (a key of ``LAUNCH_MODES``) and whether the
        sampler is outside the updated-graph mode because the process's budget of graph parameter updates was spent."""
        fb = C.c_int(0)
        return int(self._L.kmc_sampler_launch_mode(self._h, C.byref(fb))), bool(fb.value)

    def p2p_export(self) -> bytes:
        """IPC handle blob of this shard (to be all-gathered across the ranks)."""
        buf = C.create_string_buffer(_lib.P2P_HANDLE_BYTES)
        _lib.check(self._L.kmc_sampler_p2p_export(self._h, buf))
        return buf.raw

    def p2p_connect(self, blobs):
        """``blobs``: the export blobs of all ``shard_count`` ranks, in rank order."""
        raw = b"".join(bytes(b) for b in blobs)
        assert len(raw) == _lib.P2P_HANDLE_BYTES * self.cfg.shard_count
        buf = C.create_string_buffer(raw, len(raw))
        _lib.check(self._L.kmc_sampler_p2p_connect(self._h, buf))

    # -- dealt sub-ensembles (kmc_config.deal_count; see include/kissmcmc_hip.h) ---------------
    def deal_pack(self, epoch: int, send_ptr: int):
        """Enqueue the packing of this sub-ensemble's rows ([nwalkers][ndim + 2] doubles, shuffled for the deal of ``epoch``)."""
        _lib.check(self._L.kmc_sampler_deal_pack(self._h, int(epoch), C.c_void_p(send_ptr)))

    def deal_unpack(self, recv_ptr: int):
        _lib.check(self._L.kmc_sampler_deal_unpack(self._h, C.c_void_p(recv_ptr)))

    def walker_ids(self) -> np.ndarray:
        """Global walker index held by each local slot (row order of positions / naccept)."""
        out = np.empty(self.nrows, dtype=np.int64)
        _lib.check(self._L.kmc_sampler_get_walker_ids(self._h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def set_walker_ids(self, ids):
        """Dealt sub-ensembles, after :meth:`restore`: the global walker each slot holds (``distributed.deal_slot_ids``)."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(self.nrows))
        _lib.check(self._L.kmc_sampler_set_walker_ids(self._h, ids.ctypes.data_as(C.POINTER(C.c_int64))))

    def set_positions(self, theta):
        """``[nwalkers, ndim]``; a tempered sampler copies it to every rung, or takes ``[ntemps, nwalkers, ndim]``."""
        theta = np.asarray(theta, dtype=np.float64)
        if self.betas0 is not None and theta.ndim == 3:
            theta = np.ascontiguousarray(theta.reshape(self.ntemps, self.nwalkers, self.ndim))
            _lib.check(self._L.kmc_sampler_set_rung_state(self._h, _dp(theta), None, None, None, None, 0))
            return
        theta = np.ascontiguousarray(theta.reshape(self.nwalkers, self.ndim))
        self._check_host(self._L.kmc_sampler_set_positions(self._h, _dp(theta)))

    # -- parallel tempering: the whole ladder (leading axis: the rung) -------------------------
    def _need_ladder(self):
        if self.betas0 is None:
            raise ValueError("this sampler was created without parallel tempering (betas= / ntemps=)")

    def _rung_state(self, pos=False, logp=False, naccept=False, logp_sum=False):
        self._need_ladder()
        T, nw = self.ntemps, self.nwalkers
        p = np.empty((T, nw, self.ndim)) if pos else None
        lp = np.empty((T, nw)) if logp else None
        na = np.empty((T, nw), dtype=np.int64) if naccept else None
        ls = np.empty(T) if logp_sum else None
        _lib.check(self._L.kmc_sampler_get_rung_state(self._h, None if p is None else _dp(p), None if lp is None else _dp(lp),
                                                      None if na is None else na.ctypes.data_as(C.POINTER(C.c_int64)),
                                                      None if ls is None else _dp(ls)))
        return p, lp, na, ls

    def _ladder(self):
        """``(betas [T], S [T - 2], round_acc [T - 1], skipped)`` as the device holds them (kmc_sampler_get_ladder)."""
        self._need_ladder()
        T = self.ntemps
        b, S = np.zeros(T), np.zeros(max(T - 2, 0))
        ra, sk = np.zeros(T - 1, dtype=np.uint64), C.c_uint64(0)
        _lib.check(self._L.kmc_sampler_get_ladder(self._h, _dp(b), _dp(S) if T > 2 else None, ra.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(sk)))
        return b, S, ra, int(sk.value)

    @property
    def betas(self):
        """The ladder: the array given at creation, or, with ``adapt=``, the current one read from the device (frozen from
        ``adapt_until`` on; :attr:`betas0` stays the initial ladder).  ``None`` without tempering."""
        if not self.adapt or self._h is None:
            return self.betas0
        return self._ladder()[0]

    @property
    def adapt_skipped(self) -> int:
        """Rounds whose ladder update was not committed (it would not have left the ladder strictly decreasing)."""
        return self._ladder()[3]

    def rung_positions(self) -> np.ndarray:
        """``[ntemps, nwalkers, ndim]``: every rung's ensemble (rung 0 is :meth:`positions`)."""
        return self._rung_state(pos=True)[0]

    def rung_logp(self) -> np.ndarray:
        """``[ntemps, nwalkers]``: the UNTEMPERED log-density of every walker of every rung."""
        return self._rung_state(logp=True)[1]

    def rung_naccept(self) -> np.ndarray:
        """``[ntemps, nwalkers]`` accepted moves per slot since the end of burn-in (a swap leaves the counter with its slot)."""
        return self._rung_state(naccept=True)[2]

    def nswap(self) -> np.ndarray:
        """``[ntemps - 1]`` accepted exchanges between rungs ``t`` and ``t + 1`` since the end of burn-in."""
        self._need_ladder()
        out = np.zeros(self.ntemps - 1, dtype=np.uint64)
        _lib.check(self._L.kmc_sampler_get_swaps(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def swap_attempts(self) -> np.ndarray:
        """``[ntemps - 1]`` exchanges attempted per pair since the end of burn-in: it follows from the schedule (sweep ``n`` after
        generation ``g`` when ``(g + 1) % swap_every == 0``, pairs ``(t, t + 1)`` with ``t == n (mod 2)``, every walker index once)."""
        self._need_ladder()
        se, out = int(self.cfg.swap_every), np.zeros(self.ntemps - 1, dtype=np.int64)
        if se > 0:
            n_all = self.generation // se                               # sweeps so far: n = 0 .. n_all - 1, after generation (n + 1) se - 1
            n_burn = min(n_all, int(self.cfg.nburnin) // se)            # ... of which these came before counting began (g < nburnin)
            for par in (0, 1):
                cnt = (n_all + 1 - par) // 2 - (n_burn + 1 - par) // 2  # sweeps n in [n_burn, n_all) with n % 2 == par
                out[par::2] = cnt * self.nwalkers
        return out

    def swap_rates(self) -> np.ndarray:
        """``[ntemps - 1]`` accepted / attempted exchanges per neighbouring pair (``nan`` where nothing was attempted)."""
        att = self.swap_attempts().astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.nswap().astype(np.float64) / att

    def rung_logp_sum(self) -> np.ndarray:
        """``[ntemps]``: sum over stored generations and walkers of the untempered log-density of the stored state."""
        return self._rung_state(logp_sum=True)[3]

    def rung_logp_mean(self) -> np.ndarray:
        """``[ntemps]``: mean untempered log-density per rung over the stored generations -- what thermodynamic integration reads."""
        post = self.generation - self.cfg.nburnin
        done = 0 if post <= 0 else min(self.nsamples, post // self.cfg.nthin)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.rung_logp_sum() / float(done * self.nwalkers)

    # -- likelihood tempering (temper="likelihood"): S, the prior, and the evidence -------------
    def _need_likelihood(self):
        if self.temper != "likelihood":
            raise ValueError("this sampler was created without likelihood tempering (a DataDensity with betas= and temper=\"likelihood\")")

    def _rung_loglike(self, like=False, prior=False, like_sum=False):
        self._need_likelihood()
        T, nw = self.ntemps, self.nwalkers
        ll = np.empty((T, nw)) if like else None
        pr = np.empty((T, nw)) if prior else None
        ls = np.empty(T) if like_sum else None
        _lib.check(self._L.kmc_sampler_get_rung_loglike(self._h, None if ll is None else _dp(ll), None if pr is None else _dp(pr),
                                                        None if ls is None else _dp(ls)))
        return ll, pr, ls

    def rung_loglike(self) -> np.ndarray:
        """``[ntemps, nwalkers]``: the log-likelihood ``S`` (the tree sum of the data terms) of every walker of every rung."""
        return self._rung_loglike(like=True)[0]

    def rung_logprior(self) -> np.ndarray:
        """``[ntemps, nwalkers]``: the log-prior of every walker of every rung; ``rung_logp() == rung_logprior() + rung_loglike()``."""
        return self._rung_loglike(prior=True)[1]

    def rung_loglike_sum(self) -> np.ndarray:
        """``[ntemps]``: sum over stored generations and walkers of ``S`` of the stored state (taken before that generation's sweep)."""
        return self._rung_loglike(like_sum=True)[2]

    def rung_loglike_mean(self) -> np.ndarray:
        """``[ntemps]``: ``<S>`` per rung over the stored generations -- the integrand of thermodynamic integration."""
        post = self.generation - self.cfg.nburnin
        done = 0 if post <= 0 else min(self.nsamples, post // self.cfg.nthin)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.rung_loglike_sum() / float(done * self.nwalkers)

    def log_evidence(self):
        """``(logZ, err)`` = :func:`thermodynamic_integration` of ``rung_loglike_mean()`` over the ladder: the trapezoid of ``<S>_beta``
        and its every-second-rung discretisation estimate.  ``logZ`` is the log-evidence of the model only when the prior body is
        NORMALISED (a log-density that integrates to one, constants included) and the ladder ends in ``beta = 0``; a ladder that stops
        at ``beta_min > 0`` leaves out the integral from 0 to ``beta_min`` (a warning says so).  ``err`` does not include the
        Monte-Carlo error of the means.  Raises unless the sampler is likelihood-tempered."""
        self._need_likelihood()
        if self.betas[-1] != 0.0:
            import warnings
            warnings.warn(f"log_evidence: the ladder ends at beta = {self.betas[-1]:g}, not 0: the thermodynamic integral starts there "
                          "(add a prior rung: betas=[..., 0.0])", stacklevel=2)
        return thermodynamic_integration(self.betas, self.rung_loglike_mean())

    def init_ball(self, theta0, ball_radius, seed: int = 0, ball_radius_halfing_steps: int = 7, ntries: int = 100):
        """Device-side ``make_theta0s`` (reference ``src/samplers.jl:311-349``): seeded Gaussian ball
        around ``theta0`` with ``pdf > -Inf``, generated and checked on the GPU; the sampler is then
        ready to run (no host ensemble, no H2D copy).

        Differs from the host-side :func:`~kissmcmc_jl_amd.make_theta0s` in two documented ways: the random stream
        (Philox keyed by ``(seed, walker)``, not a numpy generator consumed walker by walker) and the ball's shrink
        factor, which restarts at 1 for every walker here -- the host function follows the reference, where
        ``ball_radius`` is never reset (``:326``) and one walker's retries shrink the ball of all later ones.  The two
        agree in distribution whenever no walker needs more than ``ntries`` draws."""
        th = np.ascontiguousarray(np.broadcast_to(np.asarray(theta0, dtype=np.float64), (self.ndim,)))
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(ball_radius, dtype=np.float64), (self.ndim,)))
        try:
            _lib.check(self._L.kmc_sampler_init_ball(self._h, _dp(th), _dp(r), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                     int(ball_radius_halfing_steps), int(ntries)))
        except _lib.KmcError as e:
            if e.status == _lib.ERR_NONFINITE_LOGP:
                raise RuntimeError(str(e)) from e
            raise

    def state(self):
        """Checkpoint: ``dict(positions, logp, naccept, generation)`` (synchronises)."""
        if self.betas0 is not None:            # every rung, the swap counters and the log-density sums
            p, lp, na, ls = self._rung_state(True, True, True, True)
            st = dict(positions=p, logp=lp, naccept=na, generation=self.generation, nswap=self.nswap(), rung_logp_sum=ls)
            if self.temper == "likelihood":   # (S and the prior per walker are evaluated again from the positions at restore: the same bits)
                st["rung_loglike_sum"] = self.rung_loglike_sum()
            if self.adapt:                    # the ladder as it stands, a half-finished round's counts included
                st["betas"], st["S"], st["round_acc"], st["skipped"] = self._ladder()
            return st
        return dict(positions=self.positions(), logp=self.logp(), naccept=self.naccept(), generation=self.generation)

    def restore(self, state):
        """Resume from :meth:`state` of a sampler with the same configuration and seed: the continued
        run is bit-identical to an uninterrupted one (moments restart at the restored generation)."""
        if self.betas0 is not None:
            T = self.ntemps
            pos = np.ascontiguousarray(np.asarray(state["positions"], dtype=np.float64).reshape(T, self.nwalkers, self.ndim))
            lp = np.ascontiguousarray(np.asarray(state["logp"], dtype=np.float64).reshape(T, self.nwalkers))
            na = np.ascontiguousarray(np.asarray(state["naccept"], dtype=np.int64).reshape(T, self.nwalkers))
            ns = np.ascontiguousarray(np.asarray(state["nswap"], dtype=np.uint64).reshape(T - 1))
            ls = np.ascontiguousarray(np.asarray(state["rung_logp_sum"], dtype=np.float64).reshape(T))
            _lib.check(self._L.kmc_sampler_set_rung_state(self._h, _dp(pos), _dp(lp), na.ctypes.data_as(C.POINTER(C.c_int64)),
                                                          ns.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(ls), int(state["generation"])))
            if self.temper == "likelihood":
                lls = np.ascontiguousarray(np.asarray(state["rung_loglike_sum"], dtype=np.float64).reshape(T))
                _lib.check(self._L.kmc_sampler_set_rung_loglike_sum(self._h, _dp(lls)))
            if self.adapt:                    # (after set_rung_state, which starts the ladder again)
                if "S" not in state:
                    raise ValueError("restore: the state was not taken from a sampler with adapt= (it has no ladder state)")
                b = np.ascontiguousarray(np.asarray(state["betas"], dtype=np.float64).reshape(T))
                S = np.ascontiguousarray(np.asarray(state["S"], dtype=np.float64).reshape(T - 2))
                ra = np.ascontiguousarray(np.asarray(state["round_acc"], dtype=np.uint64).reshape(T - 1))
                sk = C.c_uint64(int(state["skipped"]))
                _lib.check(self._L.kmc_sampler_set_ladder(self._h, _dp(b), _dp(S), ra.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(sk)))
            return
        pos = np.ascontiguousarray(np.asarray(state["positions"], dtype=np.float64).reshape(self.nrows, self.ndim))
        lp = np.ascontiguousarray(np.asarray(state["logp"], dtype=np.float64))
        na = np.ascontiguousarray(np.asarray(state["naccept"], dtype=np.int64))
        _lib.check(self._L.kmc_sampler_set_state(self._h, _dp(pos), _dp(lp), na.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 int(state["generation"])))

    def _check_host(self, status):
        """Re-raise an exception the host log-pdf raised inside the C callback, else check the status."""
        err = getattr(self.pdf, "error", None)
        if status != _lib.OK and err is not None:
            self.pdf.error = None
            raise err
        _lib.check(status)

    def run(self, ngenerations: int):
        self._check_host(self._L.kmc_sampler_run(self._h, int(ngenerations)))

    def half_step(self, half: int):
        _lib.check(self._L.kmc_sampler_half_step(self._h, int(half)))

    def sync(self):
        _lib.check(self._L.kmc_sampler_sync(self._h))

    def last_run_ms(self) -> float:
        ms = C.c_double()
        _lib.check(self._L.kmc_sampler_last_run_ms(self._h, C.byref(ms)))
        return ms.value

    @property
    def generation(self) -> int:
        return int(self._L.kmc_sampler_generation(self._h))

    @property
    def nsamples(self) -> int:
        return int(self._L.kmc_sampler_nsamples(self._h))

    @property
    def launch_count(self) -> int:
        return int(self._L.kmc_sampler_launch_count(self._h))

    def describe(self) -> str:
        """How this sampler executes: kernel family, geometry, exchange scheme."""
        buf = C.create_string_buffer(2048)
        _lib.check(self._L.kmc_sampler_describe(self._h, buf, 2048))
        return buf.value.decode()

    def __repr__(self):
        return f"<Sampler {self.nwalkers}x{self.ndim} {self.pdf!r}: {self.describe()}>"

    def int_acorr(self, c: float = 5.0):
        """Integrated autocorrelation time per dimension of the chain stored so far, computed where it lies (on the
        device): ``(tau[ndim], nsamples / tau)``; see :func:`kissmcmc_jl_amd.int_acorr`."""
        tau = np.zeros(self.ndim)
        conv = np.zeros(self.ndim)
        dp = C.POINTER(C.c_double)
        _lib.check(self._L.kmc_sampler_int_acorr(self._h, float(c), tau.ctypes.data_as(dp), conv.ctypes.data_as(dp)))
        return tau, conv

    # -- posterior summaries of the device chain (summary.py; README "Posterior summaries") ------
    @property
    def samples_done(self) -> int:
        """Samples stored so far."""
        post = self.generation - self.cfg.nburnin
        return 0 if post <= 0 else min(self.nsamples, post // self.cfg.nthin)

    def order_stats(self, ranks, first_sample: int = 0, walkers=None, logp: bool = False):
        """Exact order statistics of the stored chain, selected on the device (``kmc_sampler_order_stats``): for each of up to 16
        0-based ``ranks`` into the ``N = (samples_done - first_sample) * len(walkers)`` selected values of every dimension, the
        element of that rank -- ``np.sort(chain[first_sample:, walkers], axis=(0, 1))[rank]`` per dimension.  Returns
        ``(theta[len(ranks), ndim], logp[len(ranks)] | None, N)``.  ``walkers``: a boolean mask or an index array (None: all)."""
        from .summary import _SamplerProvider
        p = _SamplerProvider(self, first_sample, walkers)
        th, lp = p.order_stats(np.atleast_1d(ranks), logp)
        return th, lp, p.n

    def quantiles(self, q, first_sample: int = 0, walkers=None, logp: bool = False):
        """Quantiles ``q`` per dimension of the stored chain: ``[len(q), ndim]``, with ``logp=True`` also those of the stored
        log-densities, ``[len(q)]``.  ``x_lo + frac (x_hi - x_lo)`` (:func:`kissmcmc_jl_amd.quantile_ranks`; exactly ``x_lo`` when
        ``frac == 0``) on the host from the device's two order statistics per quantile: numpy's ``linear`` method in value."""
        from .summary import _SamplerProvider, quantiles_from
        return quantiles_from(_SamplerProvider(self, first_sample, walkers), q, logp=logp)

    def map_sample(self, first_sample: int = 0, walkers=None):
        """The stored sample of the largest log-density (needs ``store_logp``): ``(theta[ndim], logp, sample, walker)``; ties go to
        the smallest sample, then the smallest walker."""
        from .summary import _SamplerProvider
        return _SamplerProvider(self, first_sample, walkers).argmax()

    def histogram(self, bins=40, range=None, dims=None, first_sample: int = 0, walkers=None, logp: bool = False, quantile_range=None):
        """1-D marginal histograms of the stored chain, counted on the device in one read of it (``kmc_sampler_histograms``):
        ``(counts[ncols, B], edges[ncols, B + 1], outside[ncols, 3])`` for the dimensions ``dims`` (all; in the order given) and, with
        ``logp=True``, the stored log-densities as the last column.  ``bins``: a count, an edge array ``[B + 1]`` or ``[ncols, B + 1]``
        (``B <= 256``); with a count the limits are ``range`` (``(lo, hi)`` or ``[ncols, 2]``), else the quantiles ``quantile_range``,
        else each column's exact minimum and maximum, and ``s.histogram(bins=B)`` is ``np.histogram(column, bins=B)``, counts and
        edges.  ``outside``: the elements below the first edge, above the last, and the NaNs.  See :func:`kissmcmc_jl_amd.histogram`."""
        from .summary import _SamplerProvider, histogram_from
        return histogram_from(_SamplerProvider(self, first_sample, walkers), bins, range, quantile_range, dims, logp)

    def corner(self, bins=32, range=None, quantile_range=None, dims=None, first_sample: int = 0, walkers=None):
        """The numbers of a corner plot from the device chain: a dict ``dims, pairs, edges, hist1d, outside, hist2d[npairs, B, B], n``
        over 2 to 16 dimensions ``dims`` (all by default) with ``B <= 64`` bins; see :func:`kissmcmc_jl_amd.corner`."""
        from .summary import _SamplerProvider, corner_from
        return corner_from(_SamplerProvider(self, first_sample, walkers), bins, range, quantile_range, dims)

    def lag_sums(self, lag0: int = 1, nlags: int = 0, first_sample: int = 0, walkers=None, split: bool = True, logp: bool = False,
                 moments: bool = True):
        """The device stage of the convergence diagnostics on the stored chain (``kmc_sampler_lag_sums``): a dict
        ``chain_mean[ncols, m], chain_var[ncols, m], lagsum[ncols, nlags], m, h``; see :func:`kissmcmc_jl_amd.lag_sums`."""
        from .chain_convergence import sampler_lag_sums
        return sampler_lag_sums(self, lag0, nlags, first_sample, walkers, split, logp, moments)

    def convergence(self, first_sample: int = 0, walkers=None, split: bool = True, logp: bool = False, max_lag=None, rank: bool = False):
        """Split-R-hat, effective sample size and Monte-Carlo standard error per dimension of the stored chain (with ``logp=True``
        also of the stored log-densities, as the last column), read on the device where it lies (``kmc_sampler_convergence``): a dict
        of columns ``mean, std, rhat, ess, mcse, lag, truncated`` and ``m``, ``h``.  Every walker is a chain (cut in two with
        ``split``); the walkers of one ensemble are not independent, so ``rhat`` over them is optimistic -- see
        :func:`kissmcmc_jl_amd.convergence` and :func:`kissmcmc_jl_amd.evaluate_convergence`.  ``rank=True`` adds the columns
        ``rhat_rank, ess_bulk, ess_tail`` of :meth:`rank_convergence`."""
        from .chain_convergence import add_rank_columns, columns, sampler_convergence_raw
        cols = columns(sampler_convergence_raw(self, first_sample, walkers, split, logp, max_lag))
        return add_rank_columns(cols, self.rank_convergence(first_sample, walkers, split, logp, max_lag)) if rank else cols

    def rank_scores(self, first_sample: int = 0, walkers=None, split: bool = True, folded: bool = False, logp: bool = False):
        """The exact ranks of the pooled draws of the stored chain and their normal scores, ranked on the device
        (``kmc_sampler_rank_scores``): a dict ``rank2[ncols, m, h], z[ncols, m, h], centre, nan_count, S, m, h``; see
        :func:`kissmcmc_jl_amd.rank_scores`."""
        from .chain_convergence import sampler_rank_scores
        return sampler_rank_scores(self, first_sample, walkers, split, folded, logp)

    def rank_convergence(self, first_sample: int = 0, walkers=None, split: bool = True, logp: bool = False, max_lag=None):
        """Rank-normalised R-hat with bulk and tail effective sample sizes of the stored chain (``kmc_sampler_rank_convergence``): a
        dict of columns ``rhat, rhat_bulk, rhat_folded, ess_bulk, ess_tail, ess_q05, ess_q95, median, q05, q95``, ``lag[4, ncols]``,
        ``truncated``, ``has_nan`` and ``m``, ``h``; see :func:`kissmcmc_jl_amd.rank_convergence`."""
        from .chain_convergence import rank_columns, sampler_rank_convergence_raw
        return rank_columns(sampler_rank_convergence_raw(self, first_sample, walkers, split, logp, max_lag))

    def quantile_mcse(self, probs, first_sample: int = 0, walkers=None, split: bool = True, logp: bool = False, max_lag=None):
        """Quantiles of the stored chain with their effective sample sizes and Monte-Carlo standard errors
        (``kmc_sampler_quantile_mcse``): a dict of ``[nprobs, ncols]`` arrays ``quantile, ess, mcse, lower, upper, T, flags`` and ``m``,
        ``h``; see :func:`kissmcmc_jl_amd.quantile_mcse`."""
        from .chain_convergence import sampler_quantile_mcse
        return sampler_quantile_mcse(self, probs, first_sample, walkers, split, logp, max_lag)

    def indicator_lags(self, thresholds, lag0: int = 1, nlags: int = 0, first_sample: int = 0, walkers=None, split: bool = True,
                       logp: bool = False):
        """The bit-packed indicators ``x <= thresholds[nprobs, ncols]`` of the stored chain and their lag counts
        (``kmc_sampler_indicator_lags``): a dict ``ones[nprobs, ncols, m], lagcount[nprobs, ncols, nlags], m, h``; see
        :func:`kissmcmc_jl_amd.indicator_lags`."""
        from .chain_convergence import sampler_indicator_lags
        return sampler_indicator_lags(self, thresholds, lag0, nlags, first_sample, walkers, split, logp)

    def hdi(self, prob=0.94, first_sample: int = 0, walkers=None, logp: bool = False):
        """Highest-density intervals of the stored chain (with ``logp=True`` the stored log-densities are the last column), sorted and
        scanned on the device where it lies (``kmc_sampler_hdi``): a dict ``lo, hi, width, start, k, n, has_nan``, arrays ``[ncols]``
        for a scalar ``prob`` and ``[nprob, ncols]`` for a sequence of up to 16; see :func:`kissmcmc_jl_amd.hdi`."""
        from .summary import _SamplerProvider, hdi_from
        return hdi_from(_SamplerProvider(self, first_sample, walkers), prob, logp)

    def covariance(self, first_sample: int = 0, walkers=None, logp: bool = False):
        """The covariance matrix of the stored chain (with ``logp=True`` the stored log-densities are the last column), summed on the
        device where it lies (``kmc_sampler_covariance``): a dict ``mean[C], cov[C, C], corr[C, C], std[C], n``; see
        :func:`kissmcmc_jl_amd.covariance`."""
        from .chain_covariance import sampler_covariance
        return sampler_covariance(self, first_sample, walkers, logp)

    def waic(self, first_sample: int = 0, thin: int = 1, walkers=None, data=None):
        """WAIC of the sampler's :class:`DataDensity` over the stored chain -- the samples ``first_sample, first_sample + thin, ...`` of
        the walkers ``walkers`` -- evaluated on the device where chain and observations lie (``kmc_sampler_pointwise_stats``): a dict
        ``elpd_waic, se, p_waic, lppd, waic, n_high, n_nan, n`` and the arrays ``lppd_j, p_waic_j, elpd_j``; with ``data=`` over held-out
        observations instead of the density's own.  See :func:`kissmcmc_jl_amd.waic`."""
        from .chain_predictive import sampler_waic
        return sampler_waic(self, first_sample, thin, walkers, data)

    def loo(self, first_sample: int = 0, thin: int = 1, walkers=None, r_eff=1.0, obs=None, workspace=None, with_info: bool = False,
            split: bool = True, max_lag=None, r_eff_j=None):
        """PSIS-LOO of the sampler's :class:`DataDensity` over the stored chain -- the samples ``first_sample, first_sample + thin, ...`` of
        the walkers ``walkers`` -- smoothed on the device (``kmc_sampler_psis_loo``): a dict ``elpd_loo, se, p_loo, looic, lppd, n, tail_len,
        n_nan, n_reff_nan, k_counts`` and the arrays ``elpd_loo_j, p_loo_j, pareto_k, n_tail_j, lppd_j, r_eff_j, tail_len_j``; ``obs =
        (first, count)`` restricts the observations.  ``r_eff`` is one number or ``"chain"``, which computes it per observation from the
        chain; ``r_eff_j`` gives it as an array with one entry per observation (``kmc_sampler_psis_loo_reff``; ``split``, ``max_lag`` as :meth:`relative_eff`).
        See :func:`kissmcmc_jl_amd.loo`."""
        from .chain_loo import sampler_loo
        return sampler_loo(self, first_sample, thin, walkers, r_eff, obs, workspace, with_info, split, max_lag, r_eff_j)

    def psis_tail(self, first_sample: int = 0, thin: int = 1, walkers=None, r_eff=1.0, obs=None, workspace=None, split: bool = True, max_lag=None,
                  r_eff_j=None):
        """The shift, the cut-off and the sorted tail of every observation, as :meth:`loo` selects them (``kmc_sampler_psis_tail``,
        ``kmc_sampler_psis_tail_reff``); ``r_eff`` and ``r_eff_j`` are :meth:`loo`'s.  See :func:`kissmcmc_jl_amd.psis_tail`."""
        from .chain_loo import sampler_psis_tail
        return sampler_psis_tail(self, first_sample, thin, walkers, r_eff, obs, workspace, split, max_lag, r_eff_j)

    def relative_eff(self, first_sample: int = 0, thin: int = 1, walkers=None, obs=None, split: bool = True, max_lag=None, workspace=None,
                     with_info: bool = False):
        """The relative efficiency of PSIS-LOO's importance weights per observation, from the stored chain (``kmc_sampler_relative_eff``):
        a dict ``r_eff_j, ess_j, lag, truncated, m, h, n``; see :func:`kissmcmc_jl_amd.relative_eff`."""
        from .chain_loo import sampler_relative_eff
        return sampler_relative_eff(self, first_sample, thin, walkers, obs, split, max_lag, workspace, with_info)

    def pointwise_weights(self, first_sample: int = 0, thin: int = 1, walkers=None, obs=None, data=None):
        """``(v, M_j)``: the series ``v[n, stop - first] = exp(l - M_j)`` of the selected rows and the observations ``obs = (first, stop)``
        and the column maxima (``kmc_sampler_pointwise_weights``); see :func:`kissmcmc_jl_amd.pointwise_weights`."""
        from .chain_loo import sampler_pointwise_weights
        return sampler_pointwise_weights(self, first_sample, thin, walkers, obs, data)

    def pointwise_loglike(self, first_sample: int = 0, thin: int = 1, walkers=None, obs=None, data=None):
        """The matrix ``l[r, j] = term(x_r, d_j)`` of the selected rows of the stored chain and the observations ``obs = (first, stop)``
        (default: all), ``[n, stop - first]`` (``kmc_sampler_pointwise_loglike``); see :func:`kissmcmc_jl_amd.pointwise_loglike`."""
        from .chain_predictive import sampler_pointwise_loglike
        return sampler_pointwise_loglike(self, first_sample, thin, walkers, obs, data)

    def summary(self, theta_true=None, names=None, eff_samples=None, convergence=False, covariance=False, hdi=None, quantile_mcse=False):
        """:func:`kissmcmc_jl_amd.summarize_run` of the device chain: median and MAP sample (``mode``; None without ``store_logp``)
        from the device, mean and std from the streaming moments when the sampler keeps them, else from the downloaded chain;
        ``convergence=True`` adds the columns ``rhat, ess, mcse`` of :meth:`convergence`, ``convergence="rank"`` also
        ``rhat_rank, ess_bulk, ess_tail``; ``covariance=True`` adds the matrices ``cov`` and ``corr`` of :meth:`covariance`;
        ``hdi=0.94`` adds the columns ``hdi_lo, hdi_hi`` of :meth:`hdi` for that probability; ``quantile_mcse=True`` adds the column
        ``median_mcse`` of :meth:`quantile_mcse`."""
        from .summary import _SamplerProvider, quantiles_from, summary_columns
        p = _SamplerProvider(self)
        median = quantiles_from(p, [0.5])[0]
        mode = p.argmax()[0] if self.cfg.flags & _lib.STORE_LOGP else None
        if self.cfg.flags & _lib.MOMENTS:
            sm, sq, n = self.moments()
            mean = sm / n
            std = np.sqrt(np.maximum(sq - sm * sm / n, 0.0) / (n - 1)) if n > 1 else np.full(self.ndim, np.nan)
        else:
            flat = self.chain(logp=False)[0].reshape(-1, self.ndim)
            mean = flat.mean(axis=0)
            std = flat.std(axis=0, ddof=1) if flat.shape[0] > 1 else np.full(self.ndim, np.nan)
        conv = self.convergence(rank=convergence == "rank") if convergence else None
        cols = summary_columns(names, median, mean, std, mode, theta_true, eff_samples, conv, None if hdi is None else self.hdi(float(hdi)))
        if quantile_mcse:
            cols["median_mcse"] = self.quantile_mcse([0.5])["mcse"][0][:self.ndim]
        if covariance:
            c = self.covariance()
            cols.update(cov=c["cov"], corr=c["corr"])
        return cols

    def device_ptr(self, which: int) -> int:
        return int(self._L.kmc_sampler_device_ptr(self._h, int(which)) or 0)

    # -- downloads --------------------------------------------------------------------------
    def positions(self) -> np.ndarray:
        out = np.empty((self.nrows, self.ndim))
        _lib.check(self._L.kmc_sampler_get_positions(self._h, _dp(out)))
        return out

    def logp(self) -> np.ndarray:
        out = np.empty(self.nrows)
        _lib.check(self._L.kmc_sampler_get_logp(self._h, _dp(out)))
        return out

    def naccept(self) -> np.ndarray:
        out = np.empty(self.nrows, dtype=np.int64)
        _lib.check(self._L.kmc_sampler_get_naccept(self._h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def accept_ratio(self) -> np.ndarray:
        out = np.empty(self.nrows)
        _lib.check(self._L.kmc_sampler_get_accept_ratio(self._h, _dp(out)))
        return out

    def moments(self):
        """``(sum[ndim], sumsq[ndim], n)`` over the samples that would be stored."""
        s = np.empty(self.ndim)
        q = np.empty(self.ndim)
        n = C.c_int64()
        _lib.check(self._L.kmc_sampler_get_moments(self._h, _dp(s), _dp(q), C.byref(n)))
        return s, q, n.value

    def blobs(self, by_walker: bool = True):
        """Stored blobs of a ``CDensity(..., nblob=m)`` sampler created with ``store_blobs=True``: ``[nwalkers, k, m]`` --
        ``blobs[w][k]``, the reference's order (``src/samplers.jl:238, :270``) -- or ``[k, nwalkers, m]`` sample-major."""
        if self.nblob <= 0:
            raise ValueError("this sampler's density returns no blobs (CDensity(..., nblob=m))")
        k = max(0, min(self.nsamples, (self.generation - self.cfg.nburnin) // self.cfg.nthin))
        out = np.empty((self.nlocal, k, self.nblob) if by_walker else (k, self.nlocal, self.nblob))
        _lib.check(self._L.kmc_sampler_get_blobs(self._h, None, _dp(out), 1 if by_walker else 0))
        return out

    def current_blobs(self):
        """The blob of every walker's current position, ``[nwalkers, m]`` (``blob0s``, ``src/samplers.jl:210, :264``)."""
        if self.nblob <= 0:
            raise ValueError("this sampler's density returns no blobs (CDensity(..., nblob=m))")
        out = np.empty((self.nrows, self.nblob))
        _lib.check(self._L.kmc_sampler_get_blobs(self._h, _dp(out), None, 0))
        return out

    def chain(self, logp: bool = True, by_walker: bool = False, out=None):
        """``(chain [nsamples_done, nlocal, ndim], chain_logp [nsamples_done, nlocal] | None)``; with ``by_walker`` in the
        reference's order, ``thetas[w][k]`` (``src/samplers.jl:219-221``): ``[nlocal, nsamples_done, ndim]`` and
        ``[nlocal, nsamples_done]``, transposed on the device (``kmc_sampler_get_chain_by_walker``; a streamed chain is
        reordered on the host).  ``out=(chain, chain_logp)``: C-contiguous float64 arrays of exactly those shapes to fill (by-walker
        read-out of a device chain) -- a caller that allocated and faulted them in while the device was sampling (``api.emcee``)."""
        ns = self.nsamples
        post = self.generation - self.cfg.nburnin
        done = 0 if post <= 0 else min(ns, post // self.cfg.nthin)
        if self._host_chain is not None or self._host_logp is not None:
            self.sync()                                   # KMC_STREAM_CHAIN: completes the copies of everything stored so far
            if self._host_by_walker:                       # streamed in the reference's order already
                ch = None if self._host_chain is None else self._host_chain[:, :done]
                lp = self._host_logp[:, :done] if (logp and self._host_logp is not None) else None
                if not by_walker:
                    ch = None if ch is None else np.ascontiguousarray(ch.transpose(1, 0, 2))
                    lp = None if lp is None else np.ascontiguousarray(lp.T)
                return ch, lp
            ch = None if self._host_chain is None else self._host_chain[:done]
            lp = self._host_logp[:done] if (logp and self._host_logp is not None) else None
            if by_walker:
                ch = None if ch is None else np.ascontiguousarray(ch.transpose(1, 0, 2))
                lp = None if lp is None else np.ascontiguousarray(lp.T)
            return ch, lp
        if by_walker:
            ch = lp = None
            if out is not None:
                ch, lp = out
                ok = (isinstance(ch, np.ndarray) and ch.dtype == np.float64 and ch.flags.c_contiguous and ch.shape == (self.nlocal, done, self.ndim) and
                      (not logp or (isinstance(lp, np.ndarray) and lp.dtype == np.float64 and lp.flags.c_contiguous and lp.shape == (self.nlocal, done))))
                if not ok:
                    raise ValueError("out: C-contiguous float64 arrays of shapes (nlocal, samples_done, ndim) and (nlocal, samples_done)")
            else:
                ch = np.empty((self.nlocal, done, self.ndim))
                lp = np.empty((self.nlocal, done)) if logp else None
            _lib.check(self._L.kmc_sampler_get_chain_by_walker(self._h, _dp(ch), _dp(lp) if logp else None))
            return ch, (lp if logp else None)
        ch = np.empty((done, self.nlocal, self.ndim))
        lp = np.empty((done, self.nlocal)) if logp else None
        _lib.check(self._L.kmc_sampler_get_chain(self._h, _dp(ch), _dp(lp) if logp else None))
        return ch, lp
