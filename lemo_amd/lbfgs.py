"""L-BFGS with a strong-Wolfe line search: the optimiser ``optim_type: 'lbfgsls'`` selects in the PROX configs
(``temp_prox/optimizers/lbfgs_ls.py``, "use this one, lr=1.0, maxiters=30").

Two forms of the same algorithm:

* :class:`LBFGSLs` -- a ``torch.optim.Optimizer`` with ``step(closure)``: torch vectors in the parameters' dtype, every dot product
  and every scalar of the search in double.  The module-level twin of the native object and the yardstick of its tests; it is what
  :class:`lemo_amd.prox.ProxTemporalFitter` runs under ``optim_type='lbfgsls'``.
* :class:`NativeLBFGS` -- a thin wrapper over the C ABI's ``lemo_lbfgs_*`` (csrc/lbfgs_kernels.hip + csrc/lbfgs_host.hpp): the
  vectors stay on the device, the direction is one launch, a decision costs one small read-back.  ``ask`` / ``tell`` wait for the
  current stream (the ``float(closure())`` of the reference).

Both are written as an ask / tell machine (:class:`SearchMachine`, the Python twin of ``lemo_lbfgs::Machine``): ``open_step`` ->
``set_direction`` -> ``feed`` ... until the step is done.  A rule of our own, where the reference is undefined: a non-finite loss at
the start of a step moves nothing, ends the step and latches; a non-finite trial loss counts as "sufficient decrease failed".
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional

import numpy as np
import torch

from . import _hip
from ._engine import NativeHandle

DIRECTION, EVAL, DONE = 0, 1, 2
PHASES = ('initial', 'bracket', 'zoom')
STOPS = ('none', 'grad_start', 'flat', 'max_iter', 'max_eval', 'grad', 'step', 'loss', 'nonfinite')
TRACE_FIELDS = ('iter', 'phase', 't', 'f', 'gtd', 'max_g', 'accepted', 'stop')


def cubic_min(a, fa, da, b, fb, db, lo, hi):
    """minimiser of the cubic through (a, fa, da), (b, fb, db) clamped to [lo, hi]; the midpoint where there is none"""
    theta = da + db - 3.0 * (fa - fb) / (a - b)
    disc = theta * theta - da * db
    if not disc >= 0.0:
        return 0.5 * (lo + hi)
    root = math.sqrt(disc)
    if a <= b:
        pos = b - (b - a) * ((db + root - theta) / (db - da + 2.0 * root))
    else:
        pos = a - (a - b) * ((da + root - theta) / (da - db + 2.0 * root))
    return min(max(pos, lo), hi)


class _Pt:
    __slots__ = ('t', 'f', 'gtd', 'max_g', 'slot', 'row')

    def __init__(self, t=0.0, f=0.0, gtd=0.0, max_g=0.0, slot=0, row=-1):
        self.t, self.f, self.gtd, self.max_g, self.slot, self.row = t, f, gtd, max_g, slot, row

    def copy(self):
        return _Pt(self.t, self.f, self.gtd, self.max_g, self.slot, self.row)


class SearchMachine:
    """the decisions of one ``optimizer.step(closure)`` on scalars (csrc/lbfgs_host.hpp line for line in meaning)"""

    def __init__(self, lr=1.0, max_iter=20, max_eval=None, tolerance_grad=1e-5, tolerance_change=1e-9, c1=1e-4, c2=0.9, max_ls=25):
        self.lr, self.max_iter, self.max_eval = float(lr), int(max_iter), int(max_iter * 5 // 4 if max_eval is None else max_eval)
        self.tol_grad, self.tol_change, self.c1, self.c2, self.max_ls = tolerance_grad, tolerance_change, c1, c2, max_ls
        self.rows: List[list] = []
        self.latched = False
        self.n_iter = 0
        self.t = 0.0
        self.move: Optional[float] = None
        self.stop = 0
        self.cur, self.start, self.prev, self.trial, self.end = _Pt(), _Pt(), _Pt(), _Pt(), [_Pt(), _Pt()]
        self.zooming = self.stalled = False

    # -- bookkeeping
    def _log(self, phase, t, f, gtd, max_g):
        self.rows.append([float(self.n_iter), float(phase), t, f, gtd, max_g, 0.0, 0.0])
        return len(self.rows) - 1

    def _finish(self, why):
        self.stop = why
        for r in self.rows[self.row0:]:
            r[7] = float(why)
        return DONE

    def _next_iteration(self):
        self.iter += 1
        self.n_iter += 1
        return DIRECTION

    @property
    def first_ever(self):
        return self.n_iter == 1

    def _free_slot(self):
        if self.zooming:
            used = {self.end[0].slot, self.end[1].slot}
        else:
            used = {self.start.slot, self.prev.slot}
        return next(s for s in range(4) if s not in used)

    def _ask(self, t):
        self.trial = _Pt(t=t, slot=self._free_slot())
        return EVAL

    def _lower_end(self):
        return 0 if (not math.isfinite(self.end[1].f) or self.end[0].f <= self.end[1].f) else 1

    # -- protocol
    def open_step(self, f, max_g):
        self.row0 = len(self.rows)
        self.stop, self.f_open, self.iter, self.evals = 0, f, 0, 1
        self.cur = _Pt(0.0, f, 0.0, max_g, 0, self._log(0, 0.0, f, 0.0, max_g))
        if self.latched or not math.isfinite(f):
            self.latched = True
            return self._finish(8)
        self.rows[self.cur.row][6] = 1.0
        if max_g <= self.tol_grad:
            return self._finish(1)
        return self._next_iteration()

    def set_direction(self, gtd, sum_abs_g, max_d):
        self.t = min(1.0, 1.0 / sum_abs_g) * self.lr if self.first_ever else self.lr
        self.f_prev_iter = self.cur.f
        if gtd > -self.tol_change:
            return self._finish(2)
        self.d_norm = max_d
        self.start = self.cur.copy()
        self.start.t, self.start.gtd = 0.0, gtd
        self.prev = self.start.copy()
        self.ls_iter = self.ls_evals = 0
        self.zooming = False
        return self._ask(self.t)

    def feed(self, f, gtd, max_g):
        tr = self.trial
        tr.f, tr.gtd, tr.max_g = f, gtd, max_g
        tr.row = self._log(2 if self.zooming else 1, tr.t, f, gtd, max_g)
        self.ls_evals += 1
        armijo_fails = (not math.isfinite(f)) or f > self.start.f + self.c1 * tr.t * self.start.gtd
        curvature_ok = abs(gtd) <= -self.c2 * self.start.gtd
        if not self.zooming:
            if self.ls_iter == self.max_ls:
                return self._begin_zoom(self.start, tr)
            if armijo_fails or (self.ls_iter > 1 and f >= self.prev.f):
                return self._begin_zoom(self.prev, tr)
            if curvature_ok:
                return self._accept(tr)
            if gtd >= 0.0:
                return self._begin_zoom(self.prev, tr)
            lo, hi = tr.t + 0.01 * (tr.t - self.prev.t), 10.0 * tr.t
            t_next = cubic_min(self.prev.t, self.prev.f, self.prev.gtd, tr.t, tr.f, tr.gtd, lo, hi)
            self.prev = tr.copy()
            self.ls_iter += 1
            return self._ask(t_next)
        self.ls_iter += 1
        lo_i, hi_i = self.low, 1 - self.low
        if armijo_fails or f >= self.end[lo_i].f:
            self.end[hi_i] = tr.copy()
            self.low = self._lower_end()
        else:
            found = curvature_ok
            if not found and gtd * (self.end[hi_i].t - self.end[lo_i].t) >= 0.0:
                self.end[hi_i] = self.end[lo_i].copy()
            self.end[lo_i] = tr.copy()
            if found:
                return self._accept(self.end[self.low])
        if abs(self.end[1].t - self.end[0].t) * self.d_norm < self.tol_change:
            return self._accept(self.end[self.low])
        return self._zoom_trial()

    def _begin_zoom(self, a, b):
        self.zooming, self.stalled = True, False
        self.end = [a.copy(), b.copy()]
        self.low = self._lower_end()
        return self._zoom_trial()

    def _zoom_trial(self):
        if self.ls_iter >= self.max_iter:
            return self._accept(self.end[self.low])
        e0, e1 = self.end
        lo, hi = min(e0.t, e1.t), max(e0.t, e1.t)
        t = cubic_min(e0.t, e0.f, e0.gtd, e1.t, e1.f, e1.gtd, lo, hi)
        margin = 0.1 * (hi - lo)
        if min(hi - t, t - lo) < margin:
            if self.stalled or t >= hi or t <= lo:
                t = hi - margin if abs(t - hi) < abs(t - lo) else lo + margin
                self.stalled = False
            else:
                self.stalled = True
        else:
            self.stalled = False
        return self._ask(t)

    def _accept(self, p):
        q = p.copy()
        self.cur = q
        if q.row >= 0:
            self.rows[q.row][6] = 1.0
        self.t = self.move = q.t
        self.evals += self.ls_evals
        if self.iter == self.max_iter:
            return self._finish(3)
        if self.evals >= self.max_eval:
            return self._finish(4)
        if q.max_g <= self.tol_grad:
            return self._finish(5)
        if abs(q.t) * self.d_norm <= self.tol_change:
            return self._finish(6)
        if abs(q.f - self.f_prev_iter) < self.tol_change:
            return self._finish(7)
        return self._next_iteration()


def decisions(rows) -> list:
    """the decision sequence of a trace: (iteration, phase, accepted, stop) per evaluation"""
    return [(int(r[0]), int(r[1]), int(r[6]), int(r[7])) for r in rows]


def _dot(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() * b.double()).sum())


class LBFGSLs(torch.optim.Optimizer):
    """``LBFGS(line_search_fn='strong_Wolfe')`` of the reference as an ask / tell machine.  One parameter group, dense gradients.
    Vectors are kept in the parameters' dtype (as the reference's tensors are); products, sums and the search's scalars are double.
    ``step(closure)`` returns the loss the step started from.  ``trace`` holds one row per evaluation (``TRACE_FIELDS``);
    ``directions`` the direction of every iteration and ``points`` the evaluated points when ``record=True``."""

    def __init__(self, params, lr=1, max_iter=20, max_eval=None, tolerance_grad=1e-5, tolerance_change=1e-9, history_size=100,
                 line_search_fn='strong_Wolfe', c1=1e-4, c2=0.9, max_ls=25, record=False):
        if line_search_fn != 'strong_Wolfe':
            raise ValueError("LBFGSLs: only line_search_fn='strong_Wolfe' is supported")
        for name, v in (('lr', lr), ('tolerance_grad', tolerance_grad), ('tolerance_change', tolerance_change), ('c1', c1), ('c2', c2)):
            if not (math.isfinite(v) and v > 0):
                raise ValueError(f'LBFGSLs: {name} must be positive and finite')
        if max_iter < 1 or not 1 <= history_size:
            raise ValueError('LBFGSLs: max_iter and history_size must be at least 1')
        defaults = dict(lr=lr, max_iter=max_iter, max_eval=max_eval, tolerance_grad=tolerance_grad, tolerance_change=tolerance_change,
                        history_size=history_size, line_search_fn=line_search_fn)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError('LBFGSLs takes one parameter group')
        self._params = self.param_groups[0]['params']
        self.machine = SearchMachine(lr, max_iter, max_eval, tolerance_grad, tolerance_change, c1, c2, max_ls)
        self.history = int(history_size)
        self._Y: List[torch.Tensor] = []
        self._S: List[torch.Tensor] = []
        self._ro: List[float] = []
        self._hdiag = 1.0
        self._d = self._g_prev = None
        self._slots = [None] * 4
        self.record = record
        self.directions: List[torch.Tensor] = []
        self.points: List[torch.Tensor] = []
        self.last = {}

    @property
    def trace(self):
        return self.machine.rows

    # -- flat views
    def _flat_grad(self) -> torch.Tensor:
        return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in self._params]).clone()

    def _flat_x(self) -> torch.Tensor:
        return torch.cat([p.detach().reshape(-1) for p in self._params]).clone()

    @torch.no_grad()
    def _set_x(self, x: torch.Tensor) -> None:
        o = 0
        for p in self._params:
            p.copy_(x[o:o + p.numel()].view_as(p))
            o += p.numel()

    @staticmethod
    def _moved(x0: torch.Tensor, t: float, d: torch.Tensor) -> torch.Tensor:
        return (x0.double() + t * d.double()).to(x0.dtype)

    # -- the direction: memory update + two-loop recursion (what lbfgs_direction_kernel does in one launch)
    @torch.no_grad()
    def _direction(self, g: torch.Tensor, first: bool, t: float):
        dt = g.dtype
        ys = yy = 0.0
        if first:
            self._Y, self._S, self._ro, self._hdiag = [], [], [], 1.0
        else:
            y = g - self._g_prev
            s = self._d * torch.tensor(t, dtype=torch.float64).to(dt)
            ys, yy = _dot(y, s), _dot(y, y)
            if ys > 1e-10:
                if len(self._Y) == self.history:
                    self._Y.pop(0), self._S.pop(0), self._ro.pop(0)
                self._Y.append(y), self._S.append(s), self._ro.append(1.0 / ys)
                self._hdiag = ys / yy
        q = -g
        m = len(self._Y)
        al = [0.0] * m
        for i in range(m - 1, -1, -1):
            al[i] = _dot(self._S[i], q) * self._ro[i]
            q = (q.double() - al[i] * self._Y[i].double()).to(dt)
        r = (q.double() * self._hdiag).to(dt)
        for i in range(m):
            be = _dot(self._Y[i], r) * self._ro[i]
            r = (r.double() + (al[i] - be) * self._S[i].double()).to(dt)
        self._d, self._g_prev = r, g.clone()
        self.last = dict(ys=ys, yy=yy, hdiag=self._hdiag, count=m)
        return _dot(g, r), float(g.double().abs().sum()), float(r.double().abs().max()) if r.numel() else 0.0

    @staticmethod
    def _max_abs(g: torch.Tensor) -> float:
        v = float(g.double().abs().max())
        return float('nan') if bool(torch.isnan(g).any()) else v

    def step(self, closure: Callable[[], torch.Tensor]):
        M = self.machine
        with torch.enable_grad():
            loss0 = closure()
        f = float(loss0.detach())
        x0 = self._flat_x()
        g = self._flat_grad()
        self._slots[0] = g
        if self.record:
            self.points.append(x0.clone())
        want = M.open_step(f, self._max_abs(g))
        while want != DONE:
            if want == DIRECTION:
                if M.move is not None:
                    x0, M.move = self._moved(x0, M.move, self._d), None
                want = M.set_direction(*self._direction(self._slots[M.cur.slot], M.first_ever, M.t))
                if self.record:
                    self.directions.append(self._d.clone())
                continue
            x = self._moved(x0, M.trial.t, self._d)
            self._set_x(x)
            with torch.enable_grad():
                f = float(closure().detach())
            g = self._flat_grad()
            self._slots[M.trial.slot] = g
            if self.record:
                self.points.append(x.clone())
            want = M.feed(f, _dot(g, self._d), self._max_abs(g))
        if M.move is not None:
            x0, M.move = self._moved(x0, M.move, self._d), None
        self._set_x(x0)
        return loss0


class NativeLBFGS(NativeHandle):
    """``lemo_lbfgs_*`` over a workspace this object allocates with torch.  ``begin(x, g, f)`` / ``ask()`` / ``tell(g, f)`` with
    device tensors (``f``: a float32 tensor of one element).  ``ask`` returns ``(EVAL, x_trial)`` or ``(DONE, x_accepted)``; ``ask``
    and ``tell`` wait for the current stream."""
    _destroy, _held = 'lbfgs_destroy', ('ws',)

    def __init__(self, n: int, device, lr=1.0, max_iter=20, max_eval=None, tolerance_grad=1e-5, tolerance_change=1e-9, history_size=100,
                 c1=1e-4, c2=0.9, max_ls=25, _lib=None):
        import ctypes as C
        self.lib = lib = _lib or _hip.get_lib()
        self.n, self.device = int(n), torch.device(device)
        nbytes = lib.lbfgs_ws_bytes(self.n, int(history_size))
        if nbytes < 0:
            raise ValueError('NativeLBFGS: n must lie in 1 .. 32768 and history_size in 1 .. 128')
        self.ws = torch.zeros(int(nbytes) // 8 + 1, dtype=torch.float64, device=self.device)
        _hip.check_device(lib, self.ws)
        o = _hip.LbfgsOpts(float(lr), float(c1), float(c2), float(tolerance_grad), float(tolerance_change), int(max_iter),
                           int(max_iter * 5 // 4 if max_eval is None else max_eval), int(max_ls), int(history_size))
        self.handle = lib.lbfgs_create(self.n, C.byref(o), self.ws.data_ptr(), int(nbytes))
        if not self.handle:
            raise ValueError('NativeLBFGS: lemo_lbfgs_create refused the options (lr, c1, c2 and the tolerances must be positive and finite)')
        self.x_trial = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self._logs = None

    def log(self, rows: int):
        """keep the point and the direction of the next ``rows`` evaluations (diagnostics) -> (xlog, dlog) [rows, n]"""
        self._logs = (torch.zeros(rows, self.n, device=self.device), torch.zeros(rows, self.n, device=self.device))
        self.lib.check(self.lib.lbfgs_set_log(self.handle, self._logs[0].data_ptr(), self._logs[1].data_ptr(), int(rows)), 'lbfgs_set_log')
        return self._logs

    def begin(self, x: torch.Tensor, g: torch.Tensor, f: torch.Tensor) -> None:
        self._keep = (x, g, f)
        self.lib.check(self.lib.lbfgs_begin(self.handle, x.data_ptr(), g.data_ptr(), f.data_ptr(), self._s()), 'lbfgs_begin')

    def ask(self):
        rc = self.lib.lbfgs_ask(self.handle, self.x_trial.data_ptr(), self._s())
        if rc < 0:
            self.lib.check(-rc, 'lbfgs_ask')
        return rc, self.x_trial

    def tell(self, g: torch.Tensor, f: torch.Tensor) -> None:
        self._keep = (g, f)
        self.lib.check(self.lib.lbfgs_tell(self.handle, g.data_ptr(), f.data_ptr(), self._s()), 'lbfgs_tell')

    def trace(self) -> np.ndarray:
        """[rows, 8] float64, ``TRACE_FIELDS``"""
        return trace_of(self.lib, self.handle)


def trace_of(lib, handle) -> np.ndarray:
    n = lib.lbfgs_trace(handle, None, 0)
    if n < 0:
        lib.check(-n, 'lbfgs_trace')
    out = np.zeros((max(n, 1), 8), np.float64)
    lib.lbfgs_trace(handle, out.ctypes.data, int(n))
    return out[:n]
