"""OceanEnsemble: members of one small basin stepped together (libocn_sw ocn_ens_*).

A basin of the Black Sea's size fills a tenth of an MI355X, and its multi-step launch is bound by the
grid barrier between the steps.  An ensemble's members -- the same basin, mask and decomposition,
different initial state, forcing or bathymetry -- go as one launch per group of members, each member
with a barrier of its own inside it.  The reference runs one model per process and has no counterpart.
"""
from __future__ import annotations

import ctypes as C
import operator

import numpy as np

from . import _lib, ens_forcing_rule, ens_local_rule, ens_obs_rule, ens_peak_rule, ens_perturb_rule, ens_record_rule
from ._lib import check, lib
from .config import BasinConfig, ParallelConfig, SWConfig
from .model import BlockInfo, OceanModel
from .ens_local_rule import taper_table  # noqa: F401  (ensemble.taper_table)
from .output import UNDEF

# the prognostic state of the shallow-water step: what OceanEnsemble.transform recombines by default
STATE = ("ssh", "sshp", "ubrtr", "ubrtrp", "vbrtr", "vbrtrp")
# the same in OceanEnsemble.perturb's groups: both leapfrog levels of a variable share one draw
STATE_GROUPS = (("ssh", "sshp"), ("ubrtr", "ubrtrp"), ("vbrtr", "vbrtrp"))
# the real(4) mask under which the step itself stores a field, by the field name's prefix (sw_stencils.h:
# SwNextStep stores ssh / sshp under lu, ubrtr / ubrtrp under lcu, vbrtr / vbrtrp under lcv; HhUpdate and HhShift
# store hhu under llu, hhv under llv and hhh under luh; hhq is h_r + ssh, an h-point field as ssh is)
_MASKS = (("ssh", "lu"), ("ubrtr", "lcu"), ("vbrtr", "lcv"), ("hhq", "lu"), ("hhu", "llu"), ("hhv", "llv"), ("hhh", "luh"))


def default_mask(name: str):
    """OceanEnsemble.perturb's mask of real(8) field `name` when the caller names none (None: no mask)."""
    for prefix, mask in _MASKS:
        if name.startswith(prefix):
            return mask
    return None


class _Member(OceanModel):
    """An OceanModel over a handle borrowed from an ensemble: every method works; close() leaves the
    context to the ensemble."""

    def __init__(self, ctx, basin, sw, par, device):   # noqa: super().__init__ creates a context of its own
        L = lib()
        self.basin, self.sw, self.par = basin, sw, par
        self.rank, self.nranks, self.device = 0, 1, device
        self.field_names = _lib.R4_NAMES + _lib.R8_NAMES + (_lib.tracer_names(sw.tracer_num) if sw.use_tracers > 0 else [])
        self._mask = None
        self.ctx = ctx
        if basin.topography is not None:
            t = np.asfortranarray(basin.topography, dtype=np.float32)
            if t.shape != (basin.nx - 4, basin.ny - 4):
                raise ValueError(f"topography shape {t.shape} != (nx-4, ny-4) = {(basin.nx - 4, basin.ny - 4)}")
            self._topo = t
            check(L.ocn_ctx_set_topography(self.ctx, t.ctypes.data_as(C.c_void_p), t.size), "ocn_ctx_set_topography")
        self.blocks = []
        for k in range(L.ocn_ctx_block_count(self.ctx)):
            bi = _lib.OcnBlockInfo()
            check(L.ocn_ctx_block_info(self.ctx, k, C.byref(bi)), "ocn_ctx_block_info")
            g = bi.geom
            self.blocks.append(BlockInfo(k, bi.bm, bi.bn, g.nx_start, g.nx_end, g.ny_start, g.ny_end, g.bnd_x1,
                                         g.bnd_x2, g.bnd_y1, g.bnd_y2, g.pitch, tuple(bi.nbr_rank),
                                         tuple(bi.nbr_k)))

    def close(self):
        self.ctx = None


def plan(block: _lib.OcnBlock, variants, capacity: int) -> list[dict]:
    """ocn_ens_plan (pure, no device): the launch groups of members with the given variant ids
    (negative: not eligible) on `block` within `capacity` workgroups."""
    v = (C.c_int32 * len(variants))(*[int(x) for x in variants])
    n = C.c_int32(0)
    check(lib().ocn_ens_plan(C.byref(block), v, len(variants), int(capacity), None, 0, C.byref(n)), "ocn_ens_plan")
    out = (_lib.OcnEnsGroup * max(n.value, 1))()
    check(lib().ocn_ens_plan(C.byref(block), v, len(variants), int(capacity), out, n.value, C.byref(n)), "ocn_ens_plan")
    return [{"variant": int(g.variant), "rows": int(g.rows), "tiles": int(g.tiles),
             "members": [int(g.member[j]) for j in range(g.members)],
             "first_tile": [int(g.first_tile[j]) for j in range(g.members)]} for g in out[:n.value]]


class OceanEnsemble:
    """``OceanEnsemble(basin, sw, par, members, device=0)``: `members` models of one basin on one GPU.

    ``.members`` are OceanModel objects over the ensemble's contexts (upload, download, options,
    even ``step`` for one member alone); ``step`` steps them all, the members that would each run a
    multi-step launch in one launch per group."""

    def __init__(self, basin: BasinConfig, sw: SWConfig = SWConfig(), par: ParallelConfig = ParallelConfig(),
                 members: int = 1, device: int = 0):
        L = lib()
        self.basin, self.sw, self.par, self.device = basin, sw, par, device
        cb = _lib.OcnBasin(basin.nx, basin.ny, basin.dxst, basin.dyst, basin.rlon, basin.rlat, basin.curve_grid,
                           basin.rotation_on_lon, basin.rotation_on_lat)
        cs = _lib.OcnSwParams(sw.full_free_surface, sw.trans_terms, sw.ksw_lat, sw.time_smooth, sw.lvisc_2,
                              sw.use_tracers, sw.tracer_num)
        cd = _lib.OcnDecomp(par.bppnx, par.bppny, 1, 0, device)
        mptr = None
        if basin.mask is not None:
            self._mask = np.asfortranarray(basin.mask.astype(np.int32))
            if self._mask.shape != (basin.nx, basin.ny):
                raise ValueError(f"mask shape {self._mask.shape} != (nx, ny) = {(basin.nx, basin.ny)}")
            mptr = self._mask.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        self.ens = None
        check(L.ocn_ens_create(C.byref(cb), C.byref(cs), C.byref(cd), mptr, int(members), C.byref(h)), "ocn_ens_create")
        self.ens = h
        self._rec_op, self._rec_members = None, None   # (record() sets them)
        self.members: list[OceanModel] = []
        for i in range(L.ocn_ens_size(self.ens)):
            c = C.c_void_p()
            check(L.ocn_ens_member(self.ens, i, C.byref(c)), "ocn_ens_member")
            self.members.append(_Member(c, basin, sw, par, device))

    def close(self):
        if getattr(self, "ens", None):
            if getattr(self, "_recording", False):
                self.record_end()
            for m in self.members:
                m.close()
            lib().ocn_ens_destroy(self.ens)
            self.ens = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self.members)

    def init(self):
        check(lib().ocn_ens_init_state(self.ens), "ocn_ens_init_state")
        return self

    def step(self, nsteps: int = 1, tau: float = 1.0, check_every: int = 1):
        check(lib().ocn_ens_step(self.ens, tau, nsteps, check_every), "ocn_ens_step")
        return self

    def complete(self):
        check(lib().ocn_ens_complete(self.ens), "ocn_ens_complete")
        return self

    def synchronize(self, raise_on_error: bool = False) -> list[int]:
        """Wait once; the members' statuses (OCN_OK, OCN_ERR_BLOWUP, OCN_ERR_HIP).  One member's blow-up
        does not disturb the others, so by default nothing is raised."""
        st = (C.c_int32 * len(self.members))()
        rc = lib().ocn_ens_synchronize(self.ens, st)
        if raise_on_error:
            check(rc, "ocn_ens_synchronize")
        return [int(x) for x in st]

    def set_capacity(self, workgroups: int = 0):
        """A cap on the workgroups of one ensemble launch (0: none); only ever lowers the device's."""
        check(lib().ocn_ens_set_option(self.ens, _lib.ENS_OPT_CAPACITY, int(workgroups)), "ocn_ens_set_option")
        return self

    def set_max_group(self, members: int = 0):
        """Measurements: at most this many planned members are planned together (0: all), so several
        shorter launches can be timed against one taller one."""
        check(lib().ocn_ens_set_option(self.ens, _lib.ENS_OPT_MAX_GROUP, int(members)), "ocn_ens_set_option")
        return self

    def info(self) -> dict:
        """The last step(): batched launches (groups), members in them (batched), rows per wave tile, tiles
        per member and members of the largest group, and the capacity in effect."""
        i = _lib.OcnEnsInfo()
        check(lib().ocn_ens_info(self.ens, C.byref(i)), "ocn_ens_info")
        return {"members": int(i.members), "groups": int(i.groups), "batched": int(i.batched), "rows": int(i.rows),
                "tiles": int(i.tiles), "max_group": int(i.max_group), "capacity": int(i.capacity)}

    # ------------------------------------------------------------ statistics over the members
    def _use(self, members):
        """ocn_ens_stats' `use` array: None (all), or one byte per member from an iterable of indices
        (their order does not matter: the statistics run in member order)."""
        if members is None:
            return None
        use = (C.c_uint8 * len(self.members))()
        for i in members:
            if not 0 <= int(i) < len(self.members):
                raise IndexError(f"member {i} of {len(self.members)}")
            use[int(i)] = 1
        return use

    @staticmethod
    def _what(what) -> int:
        names = (what,) if isinstance(what, str) else tuple(what)
        bits = 0
        for n in names:
            bits |= _lib.ENS_STATS[n]
        return bits

    def stats(self, name: str, what=("mean", "spread"), members=None, k: int = 0) -> dict[str, np.ndarray]:
        """Per-point statistics of real(8) field `name` of block k over `members` (indices; None: all),
        formed on the device in one launch (ocn_ens_stats; the definitions are in include/ocn_sw.h):
        {statistic: float64 array of the block's array shape, Fortran order} for the names in `what`
        ("mean", "var", "spread", "min", "max").  Pending call tails of the members in use are formed first."""
        names = (what,) if isinstance(what, str) else tuple(what)
        L = lib()
        check(L.ocn_ens_stats(self.ens, k, _lib.FIELD_ID[name], self._use(members), self._what(names)), "ocn_ens_stats")
        out = {}
        for n in names:
            a = np.zeros(self.members[0].blocks[k].shape, dtype=np.float64, order="F")
            check(L.ocn_ens_stats_download(self.ens, k, _lib.ENS_STATS[n], a.ctypes.data_as(C.c_void_p)),
                  "ocn_ens_stats_download")
            out[n] = a
        return out

    def stats_output_r4(self, name: str, stat: str, k: int = 0, undef: float = float(UNDEF), members=None) -> np.ndarray:
        """The output record of one statistic of field `name` on block k's interior: real(4), `undef`
        where member 0's lu says land (ocn_ens_stats_output_r4: OceanModel.output_r4's rule and layout)."""
        L = lib()
        check(L.ocn_ens_stats(self.ens, k, _lib.FIELD_ID[name], self._use(members), _lib.ENS_STATS[stat]), "ocn_ens_stats")
        b = self.members[0].blocks[k]
        a = np.zeros((b.nx_end - b.nx_start + 1, b.ny_end - b.ny_start + 1), dtype=np.float32, order="F")
        check(L.ocn_ens_stats_output_r4(self.ens, k, _lib.ENS_STATS[stat], C.c_float(undef),
                                        a.ctypes.data_as(C.c_void_p)), "ocn_ens_stats_output_r4")
        return a

    def extrema(self, name: str) -> list[dict]:
        """Per member, over the interior sea points of real(8) field `name` on all blocks: min and max over
        the finite values (+inf / -inf with none), nonfinite (NaN, +-Inf) and count (sea points) --
        which member is about to blow up, without a download (ocn_ens_extrema).  Synchronous."""
        out = (_lib.OcnEnsExtrema * len(self.members))()
        check(lib().ocn_ens_extrema(self.ens, _lib.FIELD_ID[name], out), "ocn_ens_extrema")
        return [{"min": float(x.min), "max": float(x.max), "nonfinite": int(x.nonfinite), "count": int(x.count)}
                for x in out]

    # ------------------------------------------------------------ sampling and recombination
    def _count(self, members) -> int:
        return len(self.members) if members is None else len({int(i) for i in members})

    def sample(self, name: str, points, members=None) -> np.ndarray:
        """The members' values of real(8) field `name` at `points`, (k, i, j) triples -- local block and the
        library's 1-based global indices, anywhere in the block's array (halo and land included): a float64
        array (npts, n), column m the m-th of `members` in member order (None: all).  One launch and one wait
        (ocn_ens_sample); pending call tails of the members in use are formed first."""
        pts = np.asarray(list(points), dtype=np.int64).reshape(-1, 3)
        k, i, j = (np.ascontiguousarray(pts[:, c], dtype=np.int32) for c in range(3))
        out = np.zeros((len(pts), self._count(members)), dtype=np.float64)
        check(lib().ocn_ens_sample(self.ens, _lib.FIELD_ID[name], self._use(members), len(pts), k.ctypes.data_as(C.c_void_p),
                                   i.ctypes.data_as(C.c_void_p), j.ctypes.data_as(C.c_void_p),
                                   out.ctypes.data_as(C.c_void_p)), "ocn_ens_sample")
        return out

    def transform(self, w, names=STATE, members=None):
        """Every member in use becomes a linear combination of the members in use: new member b =
        sum over a of w[a, b] x old member a, in member order, for the real(8) fields `names` on every
        block, on the device (ocn_ens_transform; the order of operations and the treatment of zero weights
        are in include/ocn_sw.h).  `w` is an (n, n) float64 array of finite weights, n the members in use.
        The transformed fields count as uploaded: the next step forms everything derived from them again.
        Asynchronous."""
        n = self._count(members)
        a = np.asarray(w)
        if a.dtype != np.float64:
            raise TypeError(f"transform: weights of dtype {a.dtype}, not float64")
        if a.shape != (n, n):
            raise ValueError(f"transform: weights of shape {a.shape}, not {(n, n)} for {n} members in use")
        if not np.isfinite(a).all():
            raise ValueError("transform: a weight that is not finite")
        a = np.ascontiguousarray(a)
        names = (names,) if isinstance(names, str) else tuple(names)
        ids = (C.c_int32 * len(names))(*[_lib.FIELD_ID[nm] for nm in names])
        check(lib().ocn_ens_transform(self.ens, ids, len(names), self._use(members), a.ctypes.data_as(C.c_void_p)),
              "ocn_ens_transform")
        return self

    # ------------------------------------------------------------ localized observation update
    def local_update(self, y, z, obs_ij, taper, names=STATE, members=None):
        """The per-point operation of a serial square-root filter with a taper, on the device
        (ocn_ens_local_update; the rule, its order of operations and its properties are in include/ocn_sw.h):
        for one observation after another, each point of the real(8) fields `names` within the taper's reach
        is regressed on the row y[k] of observation-space anomalies and moved along z[k].  `y`, `z`: (nobs, n)
        float64 arrays of finite values, n the members in use; `obs_ij`: (nobs, 2) 1-based global indices
        within the basin; `taper`: float64 table over the squared index distance (taper_table).  At most
        8192 observations a call: a longer list is split, the calls compose bit for bit.  The updated fields
        count as uploaded.  Asynchronous."""
        n = self._count(members)
        ya, za, ta = np.asarray(y), np.asarray(z), np.asarray(taper)
        for what, a in (("y", ya), ("z", za), ("taper", ta)):
            if a.dtype != np.float64:
                raise TypeError(f"local_update: {what} of dtype {a.dtype}, not float64")
        ij = np.asarray(obs_ij)
        if ij.dtype.kind not in "iu":
            raise TypeError(f"local_update: observation indices of dtype {ij.dtype}, not integers")
        if ij.ndim != 2 or ij.shape[1] != 2 or len(ij) < 1:
            raise ValueError(f"local_update: observation indices of shape {ij.shape}, not (nobs, 2)")
        nobs = len(ij)
        if ya.shape != (nobs, n) or za.shape != (nobs, n):
            raise ValueError(f"local_update: y and z of shapes {ya.shape} and {za.shape}, not {(nobs, n)} for {nobs} "
                             f"observations and {n} members in use")
        if ta.ndim != 1 or not 1 <= len(ta) <= ens_local_rule.MAX_TAPER:
            raise ValueError(f"local_update: a taper of shape {ta.shape}, not 1..{ens_local_rule.MAX_TAPER} entries")
        if not (np.isfinite(ya).all() and np.isfinite(za).all() and np.isfinite(ta).all()):
            raise ValueError("local_update: a y, z or taper value that is not finite")
        ya, za, ta = np.ascontiguousarray(ya), np.ascontiguousarray(za), np.ascontiguousarray(ta)
        io, jo = np.ascontiguousarray(ij[:, 0], dtype=np.int32), np.ascontiguousarray(ij[:, 1], dtype=np.int32)
        names = (names,) if isinstance(names, str) else tuple(names)
        ids = (C.c_int32 * len(names))(*[_lib.FIELD_ID[nm] for nm in names])
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        check(lib().ocn_ens_local_update(self.ens, ids, len(names), self._use(members), nobs, ptr(io), ptr(jo), ptr(ya),
                                         ptr(za), ptr(ta), len(ta)), "ocn_ens_local_update")
        return self

    # ------------------------------------------------------------ inflation
    def _ids(self, names):
        names = (names,) if isinstance(names, str) else tuple(names)
        return names, (C.c_int32 * len(names))(*[_lib.FIELD_ID[nm] for nm in names])

    def spread_save(self, names=STATE, members=None):
        """Keeps the per-point spread of the real(8) fields `names` over `members` (indices; None: all, at
        least two) in buffers the ensemble owns, on every block (ocn_ens_spread_save: ocn_ens_stats' spread,
        bit for bit): the prior spread that inflate(mode="rtps") relaxes to.  No member is written.
        Asynchronous."""
        names, ids = self._ids(names)
        check(lib().ocn_ens_spread_save(self.ens, ids, len(names), self._use(members)), "ocn_ens_spread_save")
        return self

    def inflate(self, alpha: float, mode: str = "rtps", names=STATE, members=None):
        """Covariance inflation of the real(8) fields `names` over `members` on the device, per point
        (ocn_ens_inflate; the rule and its order of operations are in include/ocn_sw.h): the anomalies
        about the ensemble mean are scaled by f.  mode="const": f = alpha everywhere the members differ.
        mode="rtps" (relaxation to prior spread): f = 1 + alpha (sb - sa) / sa with sa the spread now and sb
        the one spread_save() kept for the same members, so that the new spread is alpha sb + (1 - alpha) sa;
        alpha >= 0.  A point where the members agree (land) or one holds NaN or Inf is not written.  The
        inflated fields count as uploaded.  Asynchronous."""
        if mode not in _lib.ENS_INFLATE_MODE:
            raise ValueError(f"inflate: mode {mode!r}, not one of {sorted(_lib.ENS_INFLATE_MODE)}")
        if isinstance(alpha, (str, bytes)) or np.ndim(alpha) != 0:
            raise TypeError(f"inflate: alpha {alpha!r}, not a number")
        a = float(alpha)
        if not np.isfinite(a):
            raise ValueError("inflate: an alpha that is not finite")
        if mode == "rtps" and a < 0.0:
            raise ValueError("inflate: rtps with alpha < 0")
        names, ids = self._ids(names)
        check(lib().ocn_ens_inflate(self.ens, ids, len(names), self._use(members), _lib.ENS_INFLATE_MODE[mode], a),
              "ocn_ens_inflate")
        return self

    def inflation(self, name: str, what: str = "factor", k: int = 0) -> np.ndarray:
        """What the last inflate() ("factor": the factor applied at every point of block k's array, 1.0 where
        the point was not written) or the last spread_save() ("prior_spread") left for field `name`: a
        float64 array of the block's array shape, Fortran order (ocn_ens_inflate_download).  Synchronous."""
        if what not in _lib.ENS_INFLATE_WHAT:
            raise ValueError(f"inflation: what {what!r}, not one of {sorted(_lib.ENS_INFLATE_WHAT)}")
        a = np.zeros(self.members[0].blocks[k].shape, dtype=np.float64, order="F")
        check(lib().ocn_ens_inflate_download(self.ens, k, _lib.FIELD_ID[name], _lib.ENS_INFLATE_WHAT[what],
                                             a.ctypes.data_as(C.c_void_p)), "ocn_ens_inflate_download")
        return a

    # ------------------------------------------------------------ correlated perturbations
    def perturb(self, amplitude: float, reach: int = 4, passes: int = 2, names=STATE_GROUPS, masks=None, seed: int = 0,
                draw: int = 0, centre: bool = True, members=None):
        """Adds spatially correlated random perturbations of standard deviation `amplitude` to real(8) fields
        of `members` (indices; None: all) on the device, on every block (ocn_ens_perturb; the rule is in
        include/ocn_sw.h, its numpy restatement in ens_perturb_rule.py): white integer noise from Philox4x32-10
        keyed by `seed` (0 .. 2^64-1) and counted by the global point, the member and a draw id, smoothed by
        `passes` (0..3) box sums of half-width `reach` (0..16) each way, centred over the members in use
        (centre=True: the perturbations of a point sum to zero) and added where the field's mask is set.  The
        result is bit for bit reproducible and independent of the block decomposition.
        `names`: a sequence whose entries are a field name or a tuple of names that share one draw; entry g
        gets draw id draw + g.  The default gives both leapfrog levels of a variable the same perturbation.
        `masks`: {field name: real(4) field name, or None for no mask}; a field it does not list, and every
        field with masks=None, gets default_mask(name), the mask under which the step itself stores the field.
        The perturbed fields count as uploaded.  Asynchronous."""
        if isinstance(amplitude, (str, bytes)) or np.ndim(amplitude) != 0:
            raise TypeError(f"perturb: amplitude {amplitude!r}, not a number")
        amp = float(amplitude)
        if not np.isfinite(amp) or not amp > 0.0:
            raise ValueError(f"perturb: amplitude {amplitude!r}, not finite and > 0")
        reach, passes, seed, draw = (operator.index(v) for v in (reach, passes, seed, draw))
        if not 0 <= reach <= ens_perturb_rule.MAX_REACH or not 0 <= passes <= ens_perturb_rule.MAX_PASSES:
            raise ValueError(f"perturb: reach {reach} outside 0..{ens_perturb_rule.MAX_REACH} or passes {passes} outside "
                             f"0..{ens_perturb_rule.MAX_PASSES}")
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"perturb: seed {seed} outside 0..2^64-1")
        groups = [(g,) if isinstance(g, str) else tuple(g) for g in ((names,) if isinstance(names, str) else names)]
        flat = [nm for g in groups for nm in g]
        if not flat or any(not g for g in groups):
            raise ValueError("perturb: no field, or an empty group")
        if not (0 <= draw and draw + len(groups) - 1 < 1 << 32):
            raise ValueError(f"perturb: draw ids {draw}..{draw + len(groups) - 1} outside 0..2^32-1")
        if masks is not None and set(masks) - set(flat):
            raise ValueError(f"perturb: masks for {sorted(set(masks) - set(flat))}, which are not among the fields")
        n = self._count(members)
        if n < 1 or (centre and n < 2):
            raise ValueError(f"perturb: {n} members in use" + (" with centring" if centre else ""))
        if not ens_perturb_rule.exact(n, reach, passes):
            raise ValueError(f"perturb: {n} members with reach {reach} and passes {passes}: n (2 reach + 1)^(2 passes) 2^19 "
                             f"> 2^53, not exact in double")
        mask_of = lambda nm: masks[nm] if masks is not None and nm in masks else default_mask(nm)   # noqa: E731
        mids = [-1 if mask_of(nm) is None else _lib.FIELD_ID[mask_of(nm)] for nm in flat]
        ids = (C.c_int32 * len(flat))(*[_lib.FIELD_ID[nm] for nm in flat])
        draws = (C.c_uint32 * len(flat))(*[draw + g for g, grp in enumerate(groups) for _ in grp])
        check(lib().ocn_ens_perturb(self.ens, ids, (C.c_int32 * len(flat))(*mids), draws, len(flat), self._use(members), seed,
                                    reach, passes, int(bool(centre)), amp), "ocn_ens_perturb")
        return self

    def perturbation(self, a: int, k: int = 0) -> np.ndarray:
        """Z, the smoothed integer noise before centring and scaling, of the a-th member in use from the last
        noise launch on block k (the last draw id of the last perturb()): an int64 array of the block's array
        shape, Fortran order (ocn_ens_perturb_download).  Synchronous."""
        z = np.zeros(self.members[0].blocks[k].shape, dtype=np.int64, order="F")
        check(lib().ocn_ens_perturb_download(self.ens, k, int(a), z.ctypes.data_as(C.c_void_p)), "ocn_ens_perturb_download")
        return z

    def block_of(self, i: int, j: int) -> int:
        """A local block that holds the global point (i, j): the one whose interior does, else the first
        whose array does (a point of the basin's outer rings)."""
        blocks = self.members[0].blocks
        for b in blocks:
            if b.nx_start <= i <= b.nx_end and b.ny_start <= j <= b.ny_end:
                return b.k
        for b in blocks:
            if b.bnd_x1 <= i <= b.bnd_x2 and b.bnd_y1 <= j <= b.bnd_y2:
                return b.k
        raise ValueError(f"point ({i}, {j}) lies in no local block's array")

    def assimilate(self, name: str, obs_ij, values, variances, taper, names=STATE, members=None, device: bool = False,
                   rtps=None, gate=None) -> dict:
        """A serial ensemble square-root filter (Whitaker & Hamill 2002) with localization: observations
        `values` of real(8) field `name` at the 1-based global points `obs_ij`, with error variances
        `variances`, assimilated one after another into the fields `names` of the members in use.
        sample() brings the members' values at the observed points down once; the observation-space loop
        (ens_local_rule.ensrf_obs_space) runs on the host and follows the ensemble at those points with the
        device's own rule; one local_update() does the rest on the device (several for more than 8192
        observations).  Returns {"innovations", "prior_spread", "posterior_spread", "hx"}: "hx", the (nobs, n)
        values at the observed points afterwards, is bit for bit what sample() then gives if `name` is among
        `names`.

        device=True: the whole analysis on the device (ocn_ens_assimilate: gather, observation-space loop and
        field update on the ensemble's stream, no wait in between; its sums are in member order --
        ens_local_rule.ensrf_obs_space_ordered -- so beyond a handful of members its last bits are not the
        host path's).  The same four keys, read back afterwards (one wait), plus "nonfinite", the observations
        whose innovation or innovation variance was not finite.  More than 8192 observations are split into
        calls of 8192 only if `name` is among `names` (the next call's gather then reads what the previous
        update left: the split composes); otherwise ValueError.

        rtps=alpha (a float; None: off): relaxation to prior spread around the analysis -- spread_save(names)
        before it and inflate(alpha, "rtps", names) after it, on either path; with device=True the three calls
        go out back to back with no wait in between.  The returned "hx" and "posterior_spread" describe the
        analysis BEFORE the relaxation (sample() afterwards gives the relaxed values).

        gate=sigma (a float > 0, inf allowed; None: off): quality control against the background inside the loop
        (ocn_ens_set_gate with gate2 = gate * gate; ens_local_rule.ensrf_obs_space_ordered(gate2=) restates it).  An
        observation whose squared innovation exceeds gate2 times the innovation variance of the CURRENT row, or
        whose innovation or innovation variance is not finite, is rejected: it changes no row and no field.  The
        test depends on the order of the observations, like the loop.  The returned dict gains "accepted" (a
        bool array) and "rejected" (their number).  device=True sets the ensemble's gate before every call (off
        without `gate`: a gate never leaks into a later call); device=False runs the gated loop on the host and
        passes only the accepted observations to local_update().  TypeError for a gate that is not a number,
        ValueError for one that is not > 0."""
        gate2 = ens_local_rule.gate2_of(gate, "assimilate")
        if rtps is not None:
            alpha = float(rtps)
            if not np.isfinite(alpha) or alpha < 0.0:
                raise ValueError(f"assimilate: rtps = {rtps!r}, not a finite float >= 0")
            self.spread_save(names, members=members)
            info = (self._assimilate_device(name, obs_ij, values, variances, taper, names, members, defer=True, gate2=gate2)
                    if device else
                    self.assimilate(name, obs_ij, values, variances, taper, names=names, members=members, gate=gate))
            self.inflate(alpha, "rtps", names, members=members)
            return info() if device else info
        if device:
            return self._assimilate_device(name, obs_ij, values, variances, taper, names, members, gate2=gate2)
        ij = np.asarray(obs_ij, dtype=np.int64).reshape(-1, 2)
        hx = self.sample(name, [(self.block_of(int(i), int(j)), int(i), int(j)) for i, j in ij], members=members)
        Y, Z, info = ens_local_rule.ensrf_obs_space(hx, ij, values, variances, taper, gate2=gate2)
        if gate2 is not None:   # (a rejected observation forms nothing: the update never sees it)
            Y, Z, ij = Y[info["accepted"]], Z[info["accepted"]], ij[info["accepted"]]
        for k0 in range(0, len(ij), ens_local_rule.MAX_OBS):
            k1 = k0 + ens_local_rule.MAX_OBS
            self.local_update(Y[k0:k1], Z[k0:k1], ij[k0:k1], np.asarray(taper, dtype=np.float64), names=names, members=members)
        return info

    def _set_gate(self, gate2):
        """ocn_ens_set_gate ahead of a device call: the call's own gate, or off."""
        check(lib().ocn_ens_set_gate(self.ens, 0.0 if gate2 is None else gate2), "ocn_ens_set_gate")

    def _gate_results(self, nobs: int):
        """The last device call's ("accepted", "rejected") (ocn_ens_assimilate_result, ocn_ens_gate_info)."""
        a = np.zeros(nobs, dtype=np.float64)
        check(lib().ocn_ens_assimilate_result(self.ens, _lib.ENS_ASSIM_ACCEPTED, a.ctypes.data_as(C.c_void_p)),
              "ocn_ens_assimilate_result")
        info = _lib.OcnEnsGateInfo()
        check(lib().ocn_ens_gate_info(self.ens, C.byref(info)), "ocn_ens_gate_info")
        return a != 0.0, int(info.rejected)

    def gate_info(self) -> dict:
        """ocn_ens_gate_info: the ensemble's gate2 as set (0.0: off) and the observations the last successful
        device call rejected."""
        info = _lib.OcnEnsGateInfo()
        check(lib().ocn_ens_gate_info(self.ens, C.byref(info)), "ocn_ens_gate_info")
        return {"gate2": float(info.gate2), "rejected": int(info.rejected)}

    @staticmethod
    def _assim_args(who, nobs, values, variances, taper, names):
        """What the three device analyses coerce and check alike: (values, variances, taper) as contiguous float64
        arrays and `names` as a tuple.  `who` opens the message."""
        va = np.ascontiguousarray(np.asarray(values, dtype=np.float64).ravel())
        ra = np.ascontiguousarray(np.asarray(variances, dtype=np.float64).ravel())
        ta = np.ascontiguousarray(np.asarray(taper, dtype=np.float64))
        if len(va) != nobs or len(ra) != nobs:
            raise ValueError(f"{who}: {len(va)} values and {len(ra)} variances for {nobs} observations")
        if ta.ndim != 1 or not 1 <= len(ta) <= ens_local_rule.MAX_TAPER:
            raise ValueError(f"{who}: a taper of shape {ta.shape}, not 1..{ens_local_rule.MAX_TAPER} entries")
        return va, ra, ta, (names,) if isinstance(names, str) else tuple(names)

    def _assim_results(self, nobs, n, gate2):
        """The last device call's results (one wait each): the four arrays, "nonfinite" and, with a gate,
        "accepted" and "rejected"."""
        out = {}
        for key in ("hx", "innovations", "prior_spread", "posterior_spread"):
            a = np.zeros((nobs, n) if key == "hx" else nobs, dtype=np.float64)
            check(lib().ocn_ens_assimilate_result(self.ens, _lib.ENS_ASSIM[key], a.ctypes.data_as(C.c_void_p)),
                  "ocn_ens_assimilate_result")
            out[key] = a
        info = _lib.OcnEnsAssimInfo()
        check(lib().ocn_ens_assimilate_info(self.ens, C.byref(info)), "ocn_ens_assimilate_info")
        out["nonfinite"] = int(info.nonfinite)
        if gate2 is not None:
            out["accepted"], out["rejected"] = self._gate_results(nobs)
        return out

    def _assimilate_device(self, name, obs_ij, values, variances, taper, names, members, defer: bool = False, gate2=None):
        """assimilate(device=True).  defer: return a function that reads the results back, so that the caller
        may issue more work behind the analysis before the first wait (one call's results stay in the
        ensemble's buffers until the next ocn_ens_assimilate; a split list is read back call by call as ever)."""
        n = self._count(members)
        ij = np.asarray(obs_ij)
        if ij.dtype.kind not in "iu":
            raise TypeError(f"assimilate: observation indices of dtype {ij.dtype}, not integers")
        if ij.ndim != 2 or ij.shape[1] != 2 or len(ij) < 1:
            raise ValueError(f"assimilate: observation indices of shape {ij.shape}, not (nobs, 2)")
        nobs = len(ij)
        va, ra, ta, names = self._assim_args("assimilate", nobs, values, variances, taper, names)
        if nobs > ens_local_rule.MAX_OBS and name not in names:
            raise ValueError(f"assimilate: {nobs} observations of {name!r}, which is not among the updated fields {names}: "
                             f"calls of {ens_local_rule.MAX_OBS} would not compose")
        ids = (C.c_int32 * len(names))(*[_lib.FIELD_ID[nm] for nm in names])
        io, jo = np.ascontiguousarray(ij[:, 0], dtype=np.int32), np.ascontiguousarray(ij[:, 1], dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        L = lib()
        calls = []   # each call's results (a split list is read back call by call)
        later = defer and nobs <= ens_local_rule.MAX_OBS
        for k0 in range(0, nobs, ens_local_rule.MAX_OBS):
            k1 = min(k0 + ens_local_rule.MAX_OBS, nobs)
            i_, j_, v_, r_ = (np.ascontiguousarray(a[k0:k1]) for a in (io, jo, va, ra))
            self._set_gate(gate2)
            check(L.ocn_ens_assimilate(self.ens, _lib.FIELD_ID[name], ids, len(names), self._use(members), k1 - k0, ptr(i_),
                                       ptr(j_), ptr(v_), ptr(r_), ptr(ta), len(ta)), "ocn_ens_assimilate")
            if not later:
                calls.append(self._assim_results(k1 - k0, n, gate2))
        resampled = None
        # (a row of an earlier call that a later call's observations reach: its final values are the fields')
        if nobs > ens_local_rule.MAX_OBS:
            resampled = self.sample(name, [(self.block_of(int(i), int(j)), int(i), int(j)) for i, j in ij], members=members)

        def finish():
            if later:
                calls.append(self._assim_results(nobs, n, gate2))
            out = {k: (sum(c[k] for c in calls) if k in ("nonfinite", "rejected") else np.concatenate([c[k] for c in calls]))
                   for k in calls[0]}
            if resampled is not None:
                out["hx"] = resampled
                with np.errstate(all="ignore"):
                    out["posterior_spread"] = np.array([ens_local_rule._spread(r) for r in out["hx"]])
            return out
        return finish if defer else finish()

    # ------------------------------------------------------------ off-grid observations: a sparse linear H
    def _op_arrays(self, op):
        """The operator's CSR arrays as the library takes them (kept alive by the caller)."""
        if not isinstance(op, ens_obs_rule.ObsOperator):
            raise TypeError(f"an ens_obs_rule.ObsOperator, not {type(op).__name__}")
        return [np.ascontiguousarray(op.start, dtype=np.int32),
                np.ascontiguousarray([_lib.FIELD_ID[nm] for nm in op.tname], dtype=np.int32),
                np.ascontiguousarray(op.ti, dtype=np.int32), np.ascontiguousarray(op.tj, dtype=np.int32),
                np.ascontiguousarray(op.tw, dtype=np.float64)]

    def sample_h(self, op, members=None) -> np.ndarray:
        """The sparse linear observation operator `op` (ens_obs_rule.ObsOperator: points, bilinear, combine)
        applied to the members in use: a float64 array (nobs, n), column m the m-th of `members` in member order
        (None: all), each entry the ordered sum of include/ocn_sw.h ocn_ens_sample_h -- ens_obs_rule.apply on the
        members' downloads gives the same bits.  One launch and one wait; pending call tails of the members in
        use are formed first.  At most 65536 observations a call."""
        arrays = self._op_arrays(op)
        out = np.zeros((op.nobs, self._count(members)), dtype=np.float64)
        check(lib().ocn_ens_sample_h(self.ens, self._use(members), op.nobs, *[a.ctypes.data_as(C.c_void_p) for a in arrays],
                                     out.ctypes.data_as(C.c_void_p)), "ocn_ens_sample_h")
        return out

    def assimilate_h(self, op, values, variances, taper, names=STATE, members=None, device: bool = False, rtps=None,
                     gate=None) -> dict:
        """assimilate() for observations that are not one field at one grid point: observation j is `values[j]`,
        with error variance `variances[j]`, of row j of the sparse linear operator `op`
        (ens_obs_rule.ObsOperator) applied to the members; op.anchors[j], an integer point of the basin, is its
        localization centre -- towards the other observations and towards the fields (the true position is at
        most 0.71 cells from the nearest point).  The keys returned are assimilate()'s.

        device=False: sample_h(), the observation-space loop on the host (ens_local_rule.ensrf_obs_space at the
        anchors), one local_update() at the anchors.  device=True: ocn_ens_assimilate_h -- the operator, the loop
        and the field update on the ensemble's stream with no wait in between -- plus "nonfinite".

        The rows are an augmented state carried through the loop at their anchors.  With a taper that is 1.0
        everywhere "hx" is what sample_h() gives afterwards, to rounding; with any other taper it is not (the
        fields' update weighs each term's point by its own distance).  Calls therefore do not compose: more than
        8192 observations raise ValueError on either path and are not split.

        rtps=alpha: as in assimilate() -- spread_save(names) before, inflate(alpha, "rtps", names) after, with
        device=True no wait in between.  gate=sigma: as in assimilate() -- "accepted" and "rejected" are added."""
        gate2 = ens_local_rule.gate2_of(gate, "assimilate_h")
        if rtps is not None:
            alpha = float(rtps)
            if not np.isfinite(alpha) or alpha < 0.0:
                raise ValueError(f"assimilate_h: rtps = {rtps!r}, not a finite float >= 0")
            self.spread_save(names, members=members)
            info = self._assimilate_h(op, values, variances, taper, names, members, device, defer=True, gate2=gate2)
            self.inflate(alpha, "rtps", names, members=members)
            return info()
        return self._assimilate_h(op, values, variances, taper, names, members, device, gate2=gate2)

    def _assimilate_h(self, op, values, variances, taper, names, members, device, defer: bool = False, gate2=None):
        """assimilate_h() without the relaxation.  defer: return a function that gives the results, so that the
        caller may issue more work behind the analysis before the device path's first wait."""
        arrays = self._op_arrays(op)
        nobs, n = op.nobs, self._count(members)
        if nobs > ens_local_rule.MAX_OBS:
            raise ValueError(f"assimilate_h: {nobs} observations, more than {ens_local_rule.MAX_OBS}: the rows are an "
                             f"augmented state, calls would not compose")
        va, ra, ta, names = self._assim_args("assimilate_h", nobs, values, variances, taper, names)
        if not device:
            hx = self.sample_h(op, members=members)
            Y, Z, info = ens_local_rule.ensrf_obs_space(hx, op.anchors, va, ra, ta, gate2=gate2)
            acc = slice(None) if gate2 is None else info["accepted"]
            if gate2 is None or info["accepted"].any():   # (only the accepted observations reach the update)
                self.local_update(Y[acc], Z[acc], np.asarray(op.anchors)[acc], ta, names=names, members=members)
            return (lambda: info) if defer else info
        ids = (C.c_int32 * len(names))(*[_lib.FIELD_ID[nm] for nm in names])
        io, jo = (np.ascontiguousarray(op.anchors[:, c], dtype=np.int32) for c in range(2))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        L = lib()
        self._set_gate(gate2)
        check(L.ocn_ens_assimilate_h(self.ens, ids, len(names), self._use(members), nobs, ptr(io), ptr(jo),
                                     *[ptr(a) for a in arrays], ptr(va), ptr(ra), ptr(ta), len(ta)), "ocn_ens_assimilate_h")

        finish = lambda: self._assim_results(nobs, n, gate2)   # noqa: E731  (the call's results, one wait each)
        return finish if defer else finish()

    # ------------------------------------------------------------ station time series
    def record(self, op, every: int = 1, max_records: int = 1024, members=None):
        """Start recording station time series (ocn_ens_record_begin): after every `every`-th step counted by
        step_record() the sparse linear operator `op` (ens_obs_rule.ObsOperator, as sample_h() takes it, its
        terms over ssh, sshp, ubrtr, ubrtrp, vbrtr, vbrtrp only) is applied to the members in use (`members`:
        indices; None: all) and the (nobs, n) values become the next record, up to `max_records` of them, in
        a buffer on the device.  An earlier recorder is replaced.  TypeError for an argument of the wrong type,
        ValueError for one out of range."""
        arrays = self._op_arrays(op)
        for what, v in (("every", every), ("max_records", max_records)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"record: {what} = {v!r}, not an integer")
        ens_record_rule.check(every, max_records)
        n = self._count(members)
        if max_records * op.nobs * n * 8 > ens_record_rule.MAX_SERIES_BYTES:
            raise ValueError(f"record: {max_records} records of {op.nobs} x {n} doubles, a series above 1 GiB")
        check(lib().ocn_ens_record_begin(self.ens, self._use(members), op.nobs, *[a.ctypes.data_as(C.c_void_p) for a in arrays],
                                         int(every), int(max_records)), "ocn_ens_record_begin")
        self._recording = True
        # what sample_recorded() / assimilate_recorded() need of it: the operator (its anchors) and the members
        self._rec_op = op
        self._rec_members = None if members is None else sorted({int(i) for i in members})
        return self

    def step_record(self, nsteps: int = 1, tau: float = 1.0, check_every: int = 1):
        """step() with the recorder on (ocn_ens_step_record): the members end up exactly as after
        step(nsteps, tau, check_every), and every record that falls due in these steps is written on the way --
        by the marching launch itself where the call is one (record_info()["in_launch"]), else by a gather
        launch behind each stretch of steps.  No host wait.  Plain step() calls neither count nor record."""
        if isinstance(nsteps, bool) or not isinstance(nsteps, (int, np.integer)):
            raise TypeError(f"step_record: nsteps = {nsteps!r}, not an integer")
        if nsteps < 0:
            raise ValueError(f"step_record: nsteps = {nsteps} < 0")
        check(lib().ocn_ens_step_record(self.ens, tau, int(nsteps), check_every), "ocn_ens_step_record")
        return self

    def record_info(self) -> dict:
        """The recorder: active, nobs, n, every, max_records, steps counted, records taken, and in_launch, the
        records a marching launch wrote itself (cumulative)."""
        i = _lib.OcnEnsRecordInfo()
        check(lib().ocn_ens_record_info(self.ens, C.byref(i)), "ocn_ens_record_info")
        return {"active": bool(i.active), "nobs": int(i.nobs), "n": int(i.n), "every": int(i.every),
                "max_records": int(i.max_records), "steps": int(i.steps), "records": int(i.records),
                "in_launch": int(i.in_launch)}

    def series(self, first: int = 0, count=None) -> np.ndarray:
        """Records first .. first + count - 1 (count None: all from `first`) as a float64 array
        (records, nobs, n), column m the m-th member in use in member order (ocn_ens_record_download: one wait).
        ValueError for a range outside the records taken."""
        for what, v in (("first", first), ("count", 0 if count is None else count)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"series: {what} = {v!r}, not an integer")
        info = self.record_info()
        if not info["active"]:
            raise _lib.OcnError(_lib.OCN_ERR_STATE, "series: no recorder (record())")
        count = info["records"] - first if count is None else count
        if first < 0 or count < 0 or first + count > info["records"]:
            raise ValueError(f"series: records {first} .. {first + count - 1} of {info['records']} taken")
        out = np.zeros((count, info["nobs"], info["n"]), dtype=np.float64)
        if count:
            check(lib().ocn_ens_record_download(self.ens, int(first), int(count), out.ctypes.data_as(C.c_void_p)),
                  "ocn_ens_record_download")
        return out

    def record_end(self):
        """Stop recording and free the series (ocn_ens_record_end)."""
        self._recording = False
        check(lib().ocn_ens_record_end(self.ens), "ocn_ens_record_end")
        return self

    # ------------------------------------------------------------ observations at their own times
    def _recorded_obs(self, who, rows, at, members, max_obs):
        """What sample_recorded() and assimilate_recorded() check and resolve alike: (rows, rec, wt) as the entries
        take them, the members in effect (None: all), their columns of the series (None: all) and their number."""
        info = self.record_info()
        if not info["active"]:
            raise _lib.OcnError(_lib.OCN_ERR_STATE, f"{who}: no recorder (record())")
        ra, ta = np.asarray(rows), np.asarray(at)
        if ra.dtype.kind not in "iu":
            raise TypeError(f"{who}: rows of dtype {ra.dtype}, not integers")
        if ta.dtype.kind not in "iuf":
            raise TypeError(f"{who}: times of dtype {ta.dtype}, not numbers")
        if ra.ndim != 1 or ta.shape != ra.shape:
            raise ValueError(f"{who}: rows and times of shapes {ra.shape} and {ta.shape}, not one (nobs,)")
        rec, wt = ens_record_rule.at_steps(ta.astype(np.float64), info["every"], info["records"])
        ra, rec, wt = ens_record_rule.check_obs(ra, rec, wt, info["nobs"], info["records"], max_obs)
        held = list(range(len(self.members))) if self._rec_members is None else self._rec_members
        if members is None:
            eff, cols = self._rec_members, None
        else:
            self._use(members)   # (IndexError for an index outside the ensemble)
            eff = sorted({int(i) for i in members})
            if set(eff) - set(held):
                raise ValueError(f"{who}: members {sorted(set(eff) - set(held))}, which the recorder does not hold")
            cols = [held.index(i) for i in eff]
        n = len(held) if eff is None else len(eff)
        if n < 2:
            raise ValueError(f"{who}: {n} members in use, fewer than two")
        return ra, rec, wt, eff, cols, n

    def sample_recorded(self, rows, at, members=None) -> np.ndarray:
        """The members' equivalents of observations at their own times, from the recorder's series on the device
        (ocn_ens_record_sample; the rule is in include/ocn_sw.h, its numpy restatement is
        ens_record_rule.interp): observation j is row rows[j] of the operator record() took, at the time at[j]
        in counted steps since record() (a float: it may lie between steps and between records; a row may be named
        many times).  A float64 array (nobs, n), column m the m-th of `members` in member order (None: the
        recorder's; otherwise a subset of them, at least two).  One launch and one wait; no member is read.
        TypeError for rows or times of the wrong type, ValueError for a time outside the records taken, a row
        outside the operator, more than 65536 observations or a member the recorder does not hold."""
        ra, rec, wt, _, _, n = self._recorded_obs("sample_recorded", rows, at, members, ens_record_rule.MAX_SAMPLE_OBS)
        out = np.zeros((len(ra), n), dtype=np.float64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        check(lib().ocn_ens_record_sample(self.ens, self._use(members), len(ra), ptr(ra), ptr(rec), ptr(wt), ptr(out)),
              "ocn_ens_record_sample")
        return out

    def assimilate_recorded(self, rows, at, values, variances, taper, anchors=None, names=STATE, members=None,
                            device: bool = False, rtps=None, gate=None) -> dict:
        """assimilate_h() for observations taken during the window (first guess at appropriate time, the
        asynchronous ensemble filter of Sakov et al. 2010): observation j is `values[j]`, with error variance
        `variances[j]`, of row rows[j] of the recorded operator at the time at[j] (as in sample_recorded()); the
        members' equivalents come from the recorder's series at that time, and the resulting Y and Z are applied
        to the fields `names` as they are NOW, at `anchors` ((nobs, 2) points of the basin; None: the recorded
        operator's anchors[rows]).  The keys returned are assimilate_h()'s.

        device=False: series(), ens_record_rule.interp, the observation-space loop on the host
        (ens_local_rule.ensrf_obs_space at the anchors), one local_update().  device=True: ocn_ens_assimilate_rec
        -- the gather in time, the loop and the field update on the ensemble's stream with no wait in between --
        plus "nonfinite".  `members`: None for the recorder's, otherwise a subset of them.  The recorder stays
        active and unchanged.  The records are used as they are: one taken before an earlier analysis,
        perturbation or upload of the same window is stale, and a member that blew up has undefined columns --
        leave it out with `members`.

        rtps=alpha, gate=sigma: as in assimilate_h().  TypeError for an argument of the wrong type, ValueError
        otherwise, more than 8192 observations included."""
        who = "assimilate_recorded"
        gate2 = ens_local_rule.gate2_of(gate, who)
        if rtps is not None:
            alpha = float(rtps)
            if not np.isfinite(alpha) or alpha < 0.0:
                raise ValueError(f"{who}: rtps = {rtps!r}, not a finite float >= 0")
        ra, rec, wt, eff, cols, n = self._recorded_obs(who, rows, at, members, ens_local_rule.MAX_OBS)
        nobs = len(ra)
        ij = np.asarray(self._rec_op.anchors)[ra] if anchors is None else np.asarray(anchors)
        if ij.dtype.kind not in "iu":
            raise TypeError(f"{who}: anchors of dtype {ij.dtype}, not integers")
        if ij.shape != (nobs, 2):
            raise ValueError(f"{who}: anchors of shape {ij.shape}, not {(nobs, 2)}")
        va, ra_, ta, names = self._assim_args(who, nobs, values, variances, taper, names)
        if rtps is not None:
            self.spread_save(names, members=eff)
        if not device:
            hx = ens_record_rule.interp(self.series(), ra, rec, wt, cols)
            Y, Z, out = ens_local_rule.ensrf_obs_space(hx, ij, va, ra_, ta, gate2=gate2)
            acc = slice(None) if gate2 is None else out["accepted"]
            if gate2 is None or out["accepted"].any():   # (only the accepted observations reach the update)
                self.local_update(Y[acc], Z[acc], ij[acc], ta, names=names, members=eff)
            finish = lambda: out   # noqa: E731
        else:
            ids = (C.c_int32 * len(names))(*[_lib.FIELD_ID[nm] for nm in names])
            io, jo = (np.ascontiguousarray(ij[:, c], dtype=np.int32) for c in range(2))
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
            L = lib()
            self._set_gate(gate2)
            check(L.ocn_ens_assimilate_rec(self.ens, ids, len(names), self._use(members), nobs, ptr(io), ptr(jo), ptr(ra),
                                           ptr(rec), ptr(wt), ptr(va), ptr(ra_), ptr(ta), len(ta)), "ocn_ens_assimilate_rec")

            finish = lambda: self._assim_results(nobs, n, gate2)   # noqa: E731  (the call's results, one wait each)
        if rtps is not None:   # (behind the analysis, before the device path's first wait)
            self.inflate(alpha, "rtps", names, members=eff)
        return finish()

    # ------------------------------------------------------------ moving-storm forcing
    def set_storms(self, storms, model=None, members=None):
        """Attach a moving storm to members (ocn_ens_forcing_set; the rule is in include/ocn_sw.h, its numpy
        restatement in ens_forcing_rule.py): `storms` holds one ens_forcing_rule.Storm per member in use --
        `members` (indices; None: all) in member order, or a {member index: Storm} dict, which then names the
        members itself.  `model`: an ens_forcing_rule.ForcingModel (None: its defaults) for the whole ensemble.
        A member with a storm is forced until clear_storms(): forcing(t) and step_forced() write its RHSx / RHSy,
        it steps with the general one-pass variant and runs no pair launches.  TypeError for an argument of the
        wrong type, ValueError for a value the library refuses."""
        model = ens_forcing_rule.ForcingModel() if model is None else model
        ens_forcing_rule.check_model(model)
        if isinstance(storms, dict):
            if members is not None:
                raise ValueError("set_storms: a dict of storms names the members itself")
            idx = sorted(operator.index(i) for i in storms)
            by = {operator.index(i): s for i, s in storms.items()}
        else:
            idx = list(range(len(self.members))) if members is None else sorted({operator.index(i) for i in members})
            seq = list(storms)
            if len(seq) != len(idx):
                raise ValueError(f"set_storms: {len(seq)} storms for {len(idx)} members in use")
            by = dict(zip(idx, seq))
        if not idx:
            raise ValueError("set_storms: no member in use")
        use = self._use(idx)
        arr = (_lib.OcnEnsStorm * len(self.members))()
        for i in idx:
            ens_forcing_rule.check_storm(by[i], f"set_storms: member {i}")
            arr[i] = _lib.OcnEnsStorm(*ens_forcing_rule.storm_values(by[i]))
        cm = _lib.OcnEnsForcingModel(*ens_forcing_rule.model_values(model))
        check(lib().ocn_ens_forcing_set(self.ens, use, arr, C.byref(cm)), "ocn_ens_forcing_set")
        return self

    def clear_storms(self):
        """No member is forced any more (ocn_ens_forcing_clear); RHSx / RHSy keep the last forcing."""
        check(lib().ocn_ens_forcing_clear(self.ens), "ocn_ens_forcing_clear")
        return self

    def forcing(self, t: float):
        """RHSx / RHSy of every forced member for time t (seconds), on the device, one launch per block
        (ocn_ens_forcing_apply).  Pending call tails of the forced members are formed first; the two fields then
        count as uploaded.  Asynchronous."""
        if isinstance(t, (str, bytes, bool)) or np.ndim(t) != 0:
            raise TypeError(f"forcing: t = {t!r}, not a number")
        if not np.isfinite(float(t)):
            raise ValueError("forcing: a time that is not finite")
        check(lib().ocn_ens_forcing_apply(self.ens, float(t)), "ocn_ens_forcing_apply")
        return self

    def step_forced(self, nsteps: int, tau: float, t0: float, check_every: int = 1):
        """nsteps steps of every member, step s (0-based) of a forced member under the forcing of
        t0 + s * tau (ocn_ens_step_forced): the members end up bit for bit as after forcing(t0 + s * tau);
        step(1, tau) per step, with no host work in between.  Where the forced members' calls are multi-step
        launches that go on with an open sequence (a step() or step_forced() call before this one has opened it),
        the marching launches form the forcing themselves between their steps (forcing_info()["in_launch"]).
        Members without a storm step as in step()."""
        if isinstance(nsteps, bool) or not isinstance(nsteps, (int, np.integer)):
            raise TypeError(f"step_forced: nsteps = {nsteps!r}, not an integer")
        if nsteps < 0:
            raise ValueError(f"step_forced: nsteps = {nsteps} < 0")
        for what, v in (("tau", tau), ("t0", t0)):
            if isinstance(v, (str, bytes, bool)) or np.ndim(v) != 0:
                raise TypeError(f"step_forced: {what} = {v!r}, not a number")
            if not np.isfinite(float(v)):
                raise ValueError(f"step_forced: a {what} that is not finite")
        check(lib().ocn_ens_step_forced(self.ens, float(tau), int(nsteps), int(check_every), float(t0)), "ocn_ens_step_forced")
        return self

    def forcing_info(self) -> dict:
        """ocn_ens_forcing_info: attached (forced members), applies (forcing passes so far, step_forced's included),
        steps (steps step_forced has run) and in_launch (whether the last step_forced formed the forcing inside
        its marching launches; False: one forcing launch ahead of each step)."""
        i = _lib.OcnEnsForcingInfo()
        check(lib().ocn_ens_forcing_info(self.ens, C.byref(i)), "ocn_ens_forcing_info")
        return {"attached": int(i.attached), "in_launch": bool(i.in_launch), "applies": int(i.applies), "steps": int(i.steps)}

    def set_forcing_in_launch(self, on: bool = True):
        """Tests and measurements: off, step_forced() always takes the chunked route."""
        check(lib().ocn_ens_set_option(self.ens, _lib.ENS_OPT_FORCING_IN_LAUNCH, int(bool(on))), "ocn_ens_set_option")
        return self

    # ------------------------------------------------------------ the peak map
    def peak_begin(self, field: str = "ssh", what=("max", "min"), members=None):
        """Start following the extremes of `field` (one of ens_peak_rule.FIELDS) at every interior point of the
        members in use (`members`: indices; None: all) through the steps of step() and step_forced()
        (ocn_ens_peak_begin; the rule is in include/ocn_sw.h, its numpy restatement in ens_peak_rule.py): for each
        extreme in `what` ("max", "min") an array P of the highest / lowest value after any step so far and an
        array S of that step's number, both on the device, updated between the steps of the marching launches
        themselves where a call is one (peak_info()["in_launch"]), else by one launch behind each step.  P starts as
        the field's current value, S as 0.  An earlier peak is replaced.  TypeError for an argument of the wrong
        type, ValueError for one the library refuses."""
        ens_peak_rule.check_field(field)
        bits = ens_peak_rule.what_bits(what)
        use = self._use(members)
        if members is not None and not any(use):
            raise ValueError("peak_begin: no member in use")
        check(lib().ocn_ens_peak_begin(self.ens, use, _lib.FIELD_ID[field], bits), "ocn_ens_peak_begin")
        return self

    def peak_end(self):
        """Stop following the extremes and free their arrays (ocn_ens_peak_end)."""
        check(lib().ocn_ens_peak_end(self.ens), "ocn_ens_peak_end")
        return self

    def peak_info(self) -> dict:
        """ocn_ens_peak_info: active, field, what (names), tracked (members), steps (counted since peak_begin) and
        in_launch (the steps whose update a marching launch did itself, cumulative).  OcnError (OCN_ERR_STATE)
        while no peak is active."""
        i = _lib.OcnEnsPeakInfo()
        check(lib().ocn_ens_peak_info(self.ens, C.byref(i)), "ocn_ens_peak_info")
        return {"active": bool(i.active), "field": _lib.FIELD_ID.name(int(i.field)),
                "what": tuple(n for n, b in ens_peak_rule.WHAT.items() if i.what & b), "tracked": int(i.tracked),
                "steps": int(i.steps), "in_launch": int(i.in_launch)}

    def peak(self, member: int, k: int = 0, which: str = "max"):
        """(P, S) of one tracked member on block k for `which` ("max" or "min"): a float64 and an int32 array of the
        block's array shape, Fortran order (ocn_ens_peak_download).  Synchronous."""
        bit = ens_peak_rule.which_bit(which)
        shape = self.members[0].blocks[k].shape
        P = np.zeros(shape, dtype=np.float64, order="F")
        S = np.zeros(shape, dtype=np.int32, order="F")
        check(lib().ocn_ens_peak_download(self.ens, operator.index(member), int(k), bit, P.ctypes.data_as(C.c_void_p),
                                          S.ctypes.data_as(C.c_void_p)), "ocn_ens_peak_download")
        return P, S

    def peak_stats(self, what=("mean", "max"), which: str = "max", members=None, k: int = 0) -> dict[str, np.ndarray]:
        """stats() over the tracked members' peaks instead of a field (ocn_ens_peak_stats: the same launch over the
        P arrays of `which`): {statistic: float64 array of block k's array shape}.  `members`: None for the tracked
        ones, otherwise a subset of them."""
        names = (what,) if isinstance(what, str) else tuple(what)
        bit = ens_peak_rule.which_bit(which, "peak_stats")
        L = lib()
        check(L.ocn_ens_peak_stats(self.ens, int(k), bit, self._use(members), self._what(names)), "ocn_ens_peak_stats")
        out = {}
        for n in names:
            a = np.zeros(self.members[0].blocks[k].shape, dtype=np.float64, order="F")
            check(L.ocn_ens_stats_download(self.ens, int(k), _lib.ENS_STATS[n], a.ctypes.data_as(C.c_void_p)),
                  "ocn_ens_stats_download")
            out[n] = a
        return out

    def peak_exceed(self, threshold: float, k: int = 0, members=None) -> np.ndarray:
        """Per point of block k's array, the fraction of the members in use (None: the tracked ones; otherwise a
        subset of them) whose highest value so far exceeds `threshold` (ocn_ens_peak_exceed; a NaN peak is not
        counted): a float64 array of the block's array shape.  One launch and one wait."""
        t = ens_peak_rule.check_threshold(threshold)
        a = np.zeros(self.members[0].blocks[k].shape, dtype=np.float64, order="F")
        check(lib().ocn_ens_peak_exceed(self.ens, int(k), self._use(members), t, a.ctypes.data_as(C.c_void_p)),
              "ocn_ens_peak_exceed")
        return a

    def set_peak_in_launch(self, on: bool = True):
        """Tests and measurements: off, step() and step_forced() with a peak active always take the chunked route."""
        check(lib().ocn_ens_set_option(self.ens, _lib.ENS_OPT_PEAK_IN_LAUNCH, int(bool(on))), "ocn_ens_set_option")
        return self

    # ------------------------------------------------------------ everything that is active, in one call
    def run(self, nsteps: int, tau: float = 1.0, t0=None, check_every: int = 1):
        """nsteps steps of every member with everything that is active (ocn_ens_run): forced under the storms of
        set_storms() from time `t0` on (None: unforced) as step_forced() steps them, the recorder's due records
        written as step_record() defines them, the peaks of peak_begin() following every step.  Without a recorder
        the call is step_forced() / step() itself, with a recorder alone step_record() itself; a recorder together
        with a peak and / or a forced call runs as one marching launch per group where the call is one
        (record_info(), peak_info() and forcing_info() show the route), else chunked per step; the same bits either
        way.  TypeError for an argument of the wrong type; ValueError for nsteps < 0 or a tau or t0 that is not
        finite."""
        if isinstance(nsteps, bool) or not isinstance(nsteps, (int, np.integer)):
            raise TypeError(f"run: nsteps = {nsteps!r}, not an integer")
        if isinstance(check_every, bool) or not isinstance(check_every, (int, np.integer)):
            raise TypeError(f"run: check_every = {check_every!r}, not an integer")
        if nsteps < 0:
            raise ValueError(f"run: nsteps = {nsteps} < 0")
        for what, v in (("tau", tau),) + ((("t0", t0),) if t0 is not None else ()):
            if isinstance(v, (str, bytes, bool)) or np.ndim(v) != 0:
                raise TypeError(f"run: {what} = {v!r}, not a number")
            if not np.isfinite(float(v)):
                raise ValueError(f"run: a {what} that is not finite")
        check(lib().ocn_ens_run(self.ens, float(tau), int(nsteps), int(check_every), 0 if t0 is None else 1,
                                0.0 if t0 is None else float(t0)), "ocn_ens_run")
        return self

    def set_run_in_launch(self, on: bool = True):
        """Tests and measurements: off, run() with a recorder and a peak and / or storms always takes the chunked
        route."""
        check(lib().ocn_ens_set_option(self.ens, _lib.ENS_OPT_RUN_IN_LAUNCH, int(bool(on))), "ocn_ens_set_option")
        return self

    def set_record_in_launch(self, on: bool = True):
        """Tests and measurements: off, step_record() always takes the chunked route."""
        check(lib().ocn_ens_set_option(self.ens, _lib.ENS_OPT_RECORD_IN_LAUNCH, int(bool(on))), "ocn_ens_set_option")
        return self

    def set_assim_timing(self, on: bool = True):
        """Measurements: assimilate(device=True) records events around its two stages (assimilate_spans)."""
        check(lib().ocn_ens_set_option(self.ens, _lib.ENS_OPT_ASSIM_TIMING, int(bool(on))), "ocn_ens_set_option")
        return self

    def assimilate_spans(self) -> dict:
        """The last timed assimilate(device=True) call: the milliseconds of its observation-space launch and of
        its update launches, between events on the ensemble's stream."""
        ms = (C.c_double * 2)()
        check(lib().ocn_ens_assimilate_result(self.ens, _lib.ENS_ASSIM_SPANS, ms), "ocn_ens_assimilate_result")
        return {"obs_space_ms": float(ms[0]), "update_ms": float(ms[1])}

    def assimilate_results(self, what=("y", "z")) -> dict:
        """Arrays of the last assimilate(device=True) call (ocn_ens_assimilate_result; one wait each): any of
        "hx", "y", "z" (nobs, n) and "innovations", "prior_spread", "posterior_spread" (nobs)."""
        info = _lib.OcnEnsAssimInfo()
        check(lib().ocn_ens_assimilate_info(self.ens, C.byref(info)), "ocn_ens_assimilate_info")
        out = {}
        for key in ((what,) if isinstance(what, str) else tuple(what)):
            a = np.zeros((info.nobs, info.n) if key in ("hx", "y", "z") else info.nobs, dtype=np.float64)
            check(lib().ocn_ens_assimilate_result(self.ens, _lib.ENS_ASSIM[key], a.ctypes.data_as(C.c_void_p)),
                  "ocn_ens_assimilate_result")
            out[key] = a
        return out

    @property
    def interior_cells(self) -> int:
        return sum(m.interior_cells for m in self.members)
