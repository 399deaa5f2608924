"""slam.PosteriorEvaluation -- what a trained NFiSAM solver says about its posterior, not in the reference: densities
(`posterior_log_pdf`, `joint_log_pdf`, `joint_score`), the solver grading itself (`posterior_diagnostics`, `map_estimate`,
`posterior_ksd`, `posterior_mmd`, `posterior_transport`, and against ground truth `posterior_trajectory_error`), what the posterior holds (`posterior_summary`, `posterior_modes`, `posterior_information`, `posterior_marginal_density`), its samples moved
along the joint score (`posterior_refine`, `map_refine`), the joint density's curvature (`joint_hessian_product`,
`map_newton`, `laplace_approximation`) and Metropolis chains that make the samples asymptotically exact (`posterior_mcmc`).

A mixin of `slam.NFiSAM.NFiSAM`: the walk (`posterior_launch`, `_post_columns`, `_posterior_table`) and the solver's state
are reached through `self`.  Every public method goes through ONE front, `_eval_points`, which makes the checks that need no
device and hands back an `EvalPoints` record; the kernels then read the record's column-major matrix `St` [total_dim, n]
through the `_t` bindings of nfisam_hip.  A new evaluation starts with a call of the front, not with a copy of another's
opening lines: `_eval_points` for its points (whose record also says which columns are headings: `flags`, `cols_of`),
`_reference_front` for a reference sample set and the blocks of variables to compare, `_named` around a check that does
not know the method's name, `_places` to name a per-block result."""
import contextlib

import numpy as np
import torch

import nfisam_hip as _nh


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("slam.NFiSAM needs a ROCm device (MI355X): the flow hot path has no CPU fallback")
    return "cuda:%d" % torch.cuda.current_device()


@contextlib.contextmanager
def _named(what):
    """A ValueError raised inside is raised again with the method's name in front."""
    try:
        yield
    except ValueError as e:
        raise ValueError("%s: %s" % (what, e)) from None


# how `_check_points` words its refusals: (a missing variable, a wrong shape, ragged rows, the letter of the row count)
_SAMPLE_NOUNS = ("samples lack", "samples", "ragged samples", "n")
_REFERENCE_NOUNS = ("the reference lacks", "reference samples", "ragged reference", "m")


class EvalPoints:
    """What `_eval_points` returns: values ({variable: array}, None for points that are to be drawn), rows, pcol (variable
    -> first column), total_dim, table (the clique table when log q is evaluated, else None), device (the table's, else
    where a draw lies, else the current ROCm device: asked for on first use, so that every check comes before the device
    matters) and St, the column-major float32 device matrix [total_dim, rows] -- formed on first use and once: given values
    are laid out on their side of the bus and copied over, a draw is the walk's matrix transposed.  `cols_of(v)` are a
    variable's columns, `flags` [total_dim] bool the heading columns (from the ordering's variables, formed on first use) and
    `cols` the columns the ordering's variables take, ascending: THE answer to which columns are headings, no device."""
    __slots__ = ("values", "rows", "pcol", "total_dim", "table", "_solver", "_device", "_St", "_flags")

    def __init__(self, solver, values, rows, pcol, total_dim, table):
        self.values, self.rows, self.pcol, self.total_dim, self.table = values, rows, pcol, total_dim, table
        self._solver, self._device, self._St, self._flags = solver, None, None, None

    def cols_of(self, v):
        return np.arange(self.pcol[v], self.pcol[v] + v.dim)

    @property
    def flags(self):
        if self._flags is None:
            self._flags = np.zeros(self.total_dim, dtype=bool)
            for v in self._solver._elimination_ordering:
                self._flags[self.cols_of(v)] = [bool(c) for c in v.circular_dim_list]
        return self._flags

    @property
    def cols(self):
        used = np.zeros(self.total_dim, dtype=bool)
        for v in self._solver._elimination_ordering:
            used[self.cols_of(v)] = True
        return np.flatnonzero(used)

    @property
    def device(self):
        if self._device is None:
            if self.table is not None:
                self._device = torch.device(self.table["device"])
            else:
                self._device = self.St.device if self.values is None else torch.device(_device())
        return self._device

    @property
    def St(self):
        if self._St is None:
            values, pcol = self.values, self.pcol
            if values is None:                           # [n, total_dim] on the device, as the walk hands it back
                St = self._solver.posterior_launch(self.rows)["S"].t().contiguous()
            elif values and all(torch.is_tensor(a) for a in values.values()):
                St = torch.zeros(self.total_dim, self.rows, dtype=torch.float32, device=self.device)
                for v, a in values.items():
                    St[pcol[v]:pcol[v] + v.dim] = a.to(device=self.device, dtype=torch.float32).t()
            else:
                host = np.zeros((self.total_dim, self.rows or 0), dtype=np.float32)
                for v, a in values.items():
                    host[pcol[v]:pcol[v] + v.dim] = (a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).T
                St = torch.from_numpy(host).to(self.device)
            self._St = St
        return self._St

    def over(self, St):
        """The same record over another matrix of the same layout (a copy to refine, a selection of its points)."""
        other = EvalPoints(self._solver, self.values, int(St.shape[1]), self.pcol, self.total_dim, self.table)
        other._device, other._St, other._flags = self.device, St, self._flags
        return other


class ReferenceSet:
    """What `_reference_layout` returns: values ({variable: [m, dim] host array}), m, variables (in the order asked for), rcol
    (variable -> first column of the set's own layout: the variables side by side), width, table (the blocks of variables to
    compare: one per variable, until `_reference_front` puts its own there) and Y, the float32 matrix [m, width] -- formed
    on first use and once, as `EvalPoints.St` is."""
    __slots__ = ("values", "m", "variables", "rcol", "width", "table", "_Y")

    def __init__(self, values, m, variables):
        self.values, self.m, self.variables, self._Y = values, m, variables, None
        self.rcol, self.width, self.table = {}, 0, [(v,) for v in variables]
        for v in variables:
            self.rcol[v] = self.width
            self.width += v.dim

    @property
    def Y(self):
        if self._Y is None:
            self._Y = np.concatenate([self.values[v] for v in self.variables], axis=1).astype(np.float32)
        return self._Y

    def pairs(self, pts: EvalPoints, columns: str = "all"):
        """`table` as column pairs -> [(xcols, ycols)] int64, one per block: rows of `pts.St` and the columns of `Y` they are
        compared with; columns: "all", or "xy" for the first two of every variable."""
        def take(v):
            return np.arange(v.dim if columns == "all" else min(v.dim, 2))
        return [(np.concatenate([pts.pcol[v] + take(v) for v in blk]), np.concatenate([self.rcol[v] + take(v) for v in blk]))
                for blk in self.table]


class PosteriorEvaluation:
    # ---- the front ----------------------------------------------------------------------------------------------------------
    def _check_points(self, samples, what: str, variables=None, nouns=_SAMPLE_NOUNS, host: bool = False):
        """Validation of a sample dict: `samples` maps every variable of `variables` (default: the elimination ordering) to
        [n, dim] values (numpy or torch, extra keys ignored; `host`: brought to numpy).  -> ({variable: array}, n); ValueError
        names what is wrong, in the words of `nouns`."""
        lacks, shaped, ragged, letter = nouns
        n, values = None, {}
        for v in self._elimination_ordering if variables is None else variables:
            if v not in samples:
                raise ValueError("%s: %s variable %s" % (what, lacks, v.name))
            a = samples[v]
            if host:
                a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
            if a.ndim == 1 and v.dim == 1:
                a = a.reshape(-1, 1)
            if a.ndim != 2 or a.shape[1] != v.dim:
                raise ValueError("%s: %s of %s must be [%s, %d], got %s" % (what, shaped, v.name, letter, v.dim, tuple(a.shape)))
            if n is None:
                n = int(a.shape[0])
            elif int(a.shape[0]) != n:
                raise ValueError("%s: %s: %s has %d rows, the others %d" % (what, ragged, v.name, a.shape[0], n))
            values[v] = a
        return values, n

    def _need_graph(self, what: str, factors: bool = True):
        """RuntimeError unless variables (and, with `factors`, measurement factors) have been added and ordered."""
        if (factors and not self.physical_factors) or not self._elimination_ordering:
            raise RuntimeError("%s: no factor graph yet (run an incremental update first)" % what)

    def _need_tree(self, what: str):
        """RuntimeError unless there is a Bayes tree and every clique of it has a trained model: what a draw or log q needs."""
        tree = self._physical_bayes_tree
        if tree is None or tree.root is None:
            raise RuntimeError("%s: no Bayes tree yet (run an incremental update first)" % what)
        for clique in tree.clique_ordering():
            if clique not in self._clique_density_model:
                raise RuntimeError("%s: clique %s has no trained model yet" % (what, clique))

    def _eval_points(self, what, samples, n=None, graph=True, factors=False, log_q=False, nonempty=False) -> EvalPoints:
        """What every public evaluation calls first, in this order: the graph must exist (`graph`; with `factors`: and hold
        measurement factors), the tree must be trained (for a draw, and with `log_q` for given points too), `samples` are
        checked or -- None -- the row count of a draw is `n` (default posterior_sample_num), `nonempty` refuses 0 rows, the
        columns are assigned, with `factors` the joint table is packed (an unknown factor class raises here) and with `log_q`
        the clique table is built, which then names the device.  Nothing is launched and no device is touched."""
        if graph:
            self._need_graph(what, factors=factors)
        if samples is None or log_q:
            self._need_tree(what)
        if samples is not None:
            values, rows = self._check_points(samples, what)
        else:
            values, rows = None, int(self._args.posterior_sample_num if n is None else n)
        if nonempty and rows < 1:
            raise ValueError("%s: no points" % what)
        pcol, total_dim = self._post_columns()
        if factors:
            self._joint_terms(pcol)
        return EvalPoints(self, values, rows, pcol, total_dim, self._posterior_table() if log_q else None)

    @staticmethod
    def _need_known(what: str, v, known):
        """ValueError unless `v` is one of `known` (the elimination ordering's variables, or the assigned columns)."""
        if v not in known:
            raise ValueError("%s: variable %s is not in the elimination ordering" % (what, getattr(v, "name", v)))

    def _reference_layout(self, what, reference, variables) -> ReferenceSet:
        """A reference sample set's front: `reference` maps every one of `variables` to [m, dim] values (checked by
        `_check_points` in the reference's words, brought to numpy) -> the record of its own column layout."""
        values, m = self._check_points(reference, what, variables, _REFERENCE_NOUNS, host=True)
        return ReferenceSet(values, m, list(variables))

    def _reference_front(self, what, reference, variables, blocks, joint) -> ReferenceSet:
        """What every grader against a reference set calls after `_eval_points`, in this order: `variables` default to those of
        the ordering that `reference` holds and must not be empty, every variable named (in `blocks` too: further blocks, each a
        tuple of variables) must be in the ordering and in `reference`, a block is non-empty and of compared variables, then
        `_reference_layout` -> its record with table = the joint block (with `joint`), one block per variable, `blocks`."""
        known = set(self._elimination_ordering)
        variables = [v for v in self._elimination_ordering if v in reference] if variables is None else list(variables)
        extra = [tuple(b) for b in blocks] if blocks is not None else []
        if not variables:
            raise ValueError("%s: no variable to compare (the reference holds none of the ordering's)" % what)
        for v in variables + [v for b in extra for v in b]:
            self._need_known(what, v, known)
            if v not in reference:
                raise ValueError("%s: the reference lacks variable %s" % (what, v.name))
        for b in extra:
            if not b or any(v not in variables for v in b):
                raise ValueError("%s: a block is a non-empty tuple of compared variables" % what)
        ref = self._reference_layout(what, reference, variables)
        ref.table = ([tuple(variables)] if joint else []) + ref.table + extra
        return ref

    @staticmethod
    def _places(a, variables, joint, item=float) -> dict:
        """A vector with one value per block of `_reference_front`'s table under the names the graders return it by:
        joint (None without `joint`), marginal {variable: value}, blocks [...]."""
        k0 = 1 if joint else 0
        return dict(joint=item(a[0]) if joint else None, marginal={v: item(a[k0 + i]) for i, v in enumerate(variables)},
                    blocks=[item(x) for x in a[k0 + len(variables):]])

    # ---- the launches behind them: log q, log p, the score ---------------------------------------------------------------------
    def _joint_terms(self, pcol):
        """The table of the physical factors (numpy FACTOR_DTYPE) and its uploaded copies.  Factors are only ever added and a
        variable's rows are permanent: the table is cached and extended by the records of the factors that arrived since."""
        factors = self.physical_factors
        cache = self.__dict__.get("_joint_cache")
        if cache is None or cache["count"] > len(factors):
            cache = dict(count=0, terms=np.zeros(0, dtype=_nh.FACTOR_DTYPE), dev={})
        if cache["count"] < len(factors):
            fresh = _nh.pack_factor_terms(factors[cache["count"]:], pcol)        # NotImplementedError names the class
            cache = dict(count=len(factors), terms=np.concatenate([cache["terms"], fresh]), dev={})
        self._joint_cache = cache
        return cache

    @staticmethod
    def _joint_terms_dev(cache, device, n: int):
        """The cached table's copy on `device`: uploaded on the first call with points, kept until the table grows."""
        if device not in cache["dev"] and n:
            cache["dev"][device], = _nh.upload(cache["terms"].view(np.uint8).reshape(-1), device=device, cached=True)
        return cache["dev"].get(device)

    def _log_q_launch(self, pts: EvalPoints, per_clique: bool = False):
        t = pts.table
        K, H, B, L = t["cfg"]
        return _nh.posterior_log_density_t(t["table"], t["cols"], t["obs"], pts.St, t["max_D"], K, H, B, L, pts.device,
                                           per_clique=per_clique)

    def _joint_launch(self, pts: EvalPoints, per_factor: bool = False):
        cache = self._joint_terms(pts.pcol)
        _nh.check_factor_terms(cache["terms"], pts.total_dim)
        return _nh.factor_graph_log_density_t(cache["terms"], pts.St, pts.device, per_factor=per_factor, checked=True,
                                              terms_dev=self._joint_terms_dev(cache, pts.device, pts.rows))

    def _log_p_q(self, pts: EvalPoints):
        """The two launches behind log w = log p - log q -> (log_p float64 [n], log_q float32 [n]) on the device.  What is made
        of them differs on purpose: `posterior_diagnostics` forms the weights on the host, `_weights` on the device."""
        log_q = self._log_q_launch(pts)
        return self._joint_launch(pts), log_q

    def _score_launch(self, pts: EvalPoints):
        """Gt [total_dim, n] float64 on the device: the cached table of `_joint_terms`, its gather lists kept next to it."""
        cache = self._joint_terms(pts.pcol)
        g = cache.get("gather")
        if g is None or g["row_off"].shape[0] != pts.total_dim + 1:
            g = cache["gather"] = _nh.pack_score_gather(cache["terms"], pts.total_dim)
        return _nh.factor_graph_score_t(cache["terms"], pts.St, pts.device, gather=g,
                                        terms_dev=self._joint_terms_dev(cache, pts.device, pts.rows))

    # ---- the densities -------------------------------------------------------------------------------------------------------
    def posterior_log_pdf(self, samples, per_clique: bool = False):
        """log q(X) of the tree's posterior at n points, not in the reference: the sum over the cliques of the physical Bayes
        tree of log q_c(frontal | separator, true observations), each the clique's trained flow evaluated forward on the
        device (all cliques in one launch plus a per-point sum: nfisam_nsf_posterior_log_density).

        samples: mapping variable -> [n, dim] values (numpy or torch; the dict or LazyPosterior that `sample_posterior`
        returns is valid input); it must hold every variable of the current tree, extra keys are ignored.
        -> np.ndarray[n] float32; with per_clique=True: (total [n], terms [n, n_cliques], cliques in table order).

        The density is in the variables' own units (metres, radians) and periodic in every angle.  On the circle it is
        normalised up to the mass each clique's flow puts beyond +-pi / std of its heading columns -- negligible for the
        heading spreads SLAM produces (std << pi).  Stream-ordered on the current stream behind the fits and the walk.
        Raises RuntimeError when there is no tree (or no trained model) yet, ValueError for a missing variable or ragged n,
        before anything is launched."""
        pts = self._eval_points("posterior_log_pdf", samples, graph=False, log_q=True)
        out = self._log_q_launch(pts, per_clique=per_clique)
        if per_clique:
            log_q, per, _ = out
            return log_q.cpu().numpy(), per.t().cpu().numpy(), list(pts.table["cliques"])
        return out.cpu().numpy()

    def joint_log_pdf(self, samples, per_factor: bool = False):
        """log p(X, Z) = sum over the measurement factors f of log p_f(x_f) at n points: the reference's JointFactor.log_pdf
        (src/sampler/sampler_utils.py:85-98) over `physical_factors` -- the factors of the graph, never the FlowsPriorFactor
        messages of the working graph -- evaluated on the device in float64 at the float32 points
        (nfisam_factor_graph_log_density; mixtures by log-sum-exp, finite where the reference underflows to -inf).

        samples: as `posterior_log_pdf` (dict or LazyPosterior, numpy or torch, extra keys ignored).
        -> np.ndarray[n] float64; with per_factor=True: (total [n], terms [n, n_factors], factors in table order); the total
        is the left-to-right float64 sum of the terms.  Headings count modulo 2 pi.
        Raises RuntimeError when no factor graph has been built yet, ValueError for a missing variable, a wrong width or
        ragged n, NotImplementedError naming the class of a factor without a device code -- before anything is launched."""
        pts = self._eval_points("joint_log_pdf", samples, factors=True)
        factors = self.physical_factors
        out = self._joint_launch(pts, per_factor=per_factor)
        if per_factor:
            return out[0].cpu().numpy(), out[1].t().cpu().numpy(), list(factors)
        return out.cpu().numpy()

    def posterior_diagnostics(self, samples=None, n: int = None) -> dict:
        """The solver grading itself without ground truth: log w = log p - log q at posterior samples.

        samples=None draws `n` (default posterior_sample_num) points through the tree walk and scores the device matrix where
        it lies; otherwise `samples` is scored (as `posterior_log_pdf` / `joint_log_pdf` accept it) and nothing is drawn: the
        solver's state and random streams are untouched.
        -> dict: log_p, log_q, log_w (float64 [n]), elbo (mean log w), log_evidence (logsumexp(log w) - log n), ess
        ((sum w)^2 / sum w^2 from max-shifted weights, in [1, n]), map_index (argmax of log p over the draw: the reference's
        MAP rule, src/slam/FactorGraphSolver.py:660-671), map_sample (variable -> [dim]).

        p is the unnormalised joint p(X, Z) of the measurement factors and q a normalised density of X, so `log_evidence`
        estimates log p(Z) and `elbo` bounds it from below; headings are compared modulo 2 pi on both sides.  log_w is
        therefore not something that should average to zero.  log q is a float32 value of magnitude ~5e3 (spacing 5e-4);
        log w inherits that."""
        pts = self._eval_points("posterior_diagnostics", samples, n, factors=True, log_q=True)
        log_p, log_q = self._log_p_q(pts)
        log_p, log_q = log_p.cpu().numpy(), log_q.cpu().numpy().astype(np.float64)
        log_w = log_p - log_q
        out = dict(log_p=log_p, log_q=log_q, log_w=log_w)
        if log_w.size == 0:
            raise ValueError("posterior_diagnostics: no points")
        top = log_w.max()
        w = np.exp(log_w - top)
        out["elbo"] = float(log_w.mean())
        out["log_evidence"] = float(top + np.log(w.sum()) - np.log(log_w.size))
        out["ess"] = float(w.sum() ** 2 / (w * w).sum())
        k = int(np.argmax(log_p))
        row, pcol = pts.St[:, k].cpu().numpy(), pts.pcol
        out["map_index"] = k
        out["map_sample"] = {v: row[pcol[v]:pcol[v] + v.dim].copy() for v in self._elimination_ordering}
        return out

    def map_estimate(self, samples=None) -> dict:
        """The sample of highest joint density log p among `samples` (or a fresh posterior draw): the reference's MAP
        estimate (FactorGraphSolver.plot2d_MAP_rbt_only, src/slam/FactorGraphSolver.py:660-671).  -> variable -> [dim]."""
        return self.posterior_diagnostics(samples)["map_sample"]

    # ---- what posterior_ksd, posterior_refine and map_refine share: the spreads of the columns in use ----------------------------
    @staticmethod
    def _column_scale(pts: EvalPoints, flags, cols, standardise: bool):
        """-> scale [total_dim]: with `standardise` 1 / spread of every column of `cols` over the points of `pts`
        (`sample_moments_t` + `Statistics.mode_scale`: the circular spread for a heading, 0 for a column without spread), else
        1; 0 in the columns no variable takes."""
        from utils import Statistics as ST
        scale = np.zeros(pts.total_dim)
        if standardise:
            circ = flags[cols].astype(np.uint8)
            mean, res, cov = _nh.sample_moments_t(pts.St, _nh.pack_moment_blocks(np.ones(cols.size, dtype=np.int64)), cols,
                                                  circ if circ.any() else None, None, checked=True)
            scale[cols] = ST.mode_scale(cov.cpu().numpy(), res.cpu().numpy(), flags[cols])
        else:
            scale[cols] = 1.0
        return scale

    # ---- the solver graded against the factor graph itself: score and kernel Stein discrepancy -------------------------
    def joint_score(self, samples) -> np.ndarray:
        """The score grad_x log p(X, Z) of the measurement factors at n points: the reference's JointFactor.grad_x_log_pdf
        (src/sampler/sampler_utils.py:101-118) over `physical_factors`, on the device in float64 at the float32 points
        (nfisam_factor_graph_score: the zero vector at a range of exactly 0, softmax weights for mixtures -- finite where the
        reference divides by zero).

        samples: as `joint_log_pdf`.  -> np.ndarray [n, total_dim] float64, columns in the walk's permanent layout
        (`_post_columns`: variable -> first column).  Raises what `joint_log_pdf` raises, before anything is launched."""
        return self._score_launch(self._eval_points("joint_score", samples, factors=True)).t().cpu().numpy()

    def posterior_ksd(self, samples=None, n: int = None, sigma=None, standardise: bool = True, nboot: int = 0,
                      seed=None) -> dict:
        """The solver graded against the factor graph itself, without a second sample set: the Gaussian kernel Stein
        discrepancy (reference src/utils/Statistics.py:216-245) between posterior samples and the joint density p(X, Z)
        through its score, both evaluated on the device where the sample matrix lies (nfisam_factor_graph_score,
        nfisam_sample_ksd).

        samples=None draws `n` (default posterior_sample_num) points through the tree walk; otherwise `samples` is graded (as
        `joint_log_pdf` accepts it) and nothing is drawn.  standardise: every column's differences are divided by its spread
        (the circular standard deviation for a heading; a column without spread leaves the kernel: scale 0); sigma: the
        bandwidth in those units, None = sqrt(total_dim).  Headings are flagged circular from the variables: see
        `Statistics.kernel_stein_discrepancy` on the antipode.  nboot > 0 adds the reference's multinomial bootstrap, its draws
        from a generator of its own seeded with `seed`.
        -> dict: ustat (None for n = 1), vstat, row_mean [n] (sum_j h_ij / n per point: where the draw disagrees with the
        graph), precision (variable -> [dim]), sigma, n, and p_value / bootstrap with nboot > 0.
        Nothing of the solver's state or random streams is touched (a draw uses the walk's generator as `sample_posterior`
        does).  Raises RuntimeError when there is no graph / tree yet, NotImplementedError naming a factor class without a
        device code, ValueError for bad points or options -- before anything is launched."""
        from utils import Statistics as ST
        what = "posterior_ksd"
        pts = self._eval_points(what, samples, n, factors=True, nonempty=True)
        rows, pcol, total_dim = pts.rows, pts.pcol, pts.total_dim
        nboot = int(nboot)
        if nboot < 0 or (nboot > 0 and (rows < 2 or rows > _nh.KSD_MATRIX_MAX_N)):
            raise ValueError("%s: the bootstrap needs nboot >= 0 and 2 <= n <= %d" % (what, _nh.KSD_MATRIX_MAX_N))
        if sigma is not None and not (np.isfinite(sigma) and sigma > 0):
            raise ValueError("%s: sigma must be positive and finite" % what)
        order = list(self._elimination_ordering)
        flags, cols = pts.flags, pts.cols
        scale = self._column_scale(pts, flags, cols, standardise)
        sig = float(np.sqrt(cols.size)) if sigma is None else float(sigma)
        precision = scale * scale / (sig * sig)
        Gt = self._score_launch(pts)
        sums = _nh.ksd_sums_t(pts.St, Gt, precision, wrap=flags.astype(np.uint8) if flags.any() else None, matrix=nboot > 0)
        row = sums["row"].cpu().numpy()
        u, vstat = ST.ksd_from_sums(row.sum(), sums["diag"].cpu().numpy().sum(), rows, ustat=rows >= 2)
        out = dict(ustat=u, vstat=vstat, row_mean=row / rows, n=rows, sigma=sig,
                   precision={v: precision[pcol[v]:pcol[v] + v.dim].copy() for v in order})
        if nboot > 0:
            rng = np.random.RandomState(seed)
            draws = np.stack([rng.multinomial(rows, np.ones(rows) / rows) for _ in range(nboot)])
            out["bootstrap"] = ST.ksd_bootstrap(sums["H"], draws)
            out["p_value"] = float(np.mean(out["bootstrap"] >= u))
        return out

    # ---- the samples moved along the joint score: Stein variational refinement and a MAP ascent ----------------------------------
    def _refine_front(self, what, samples, n, steps, step_size, standardise, blocks_of, sigma=None):
        """What posterior_refine and map_refine share: the front, every option check (no device; `blocks_of(pts, cols)` makes
        the method's own and returns its column blocks), then the spreads of the starting points
        -> (pts, flags, cols, blocks, scale [total_dim], step [total_dim]).  A column's step is `step_size`
        times its spread with `standardise` (`step_size` itself for a column without spread), else `step_size`."""
        from utils import Statistics as ST
        pts = self._eval_points(what, samples, n, factors=True, nonempty=True)
        flags, cols = pts.flags, pts.cols
        blocks = blocks_of(pts, cols)
        with _named(what):
            if np.ndim(step_size) != 0:
                raise ValueError("step_size is one positive finite step")
            ST.check_refine_options(pts.total_dim, blocks, sigma, None, flags, steps, step_size)
        scale = self._column_scale(pts, flags, cols, bool(standardise))
        step = np.full(pts.total_dim, float(step_size))
        if standardise:
            step[scale > 0] = float(step_size) / scale[scale > 0]
        return pts, flags, cols, blocks, scale, step

    def _samples_of(self, St, pcol):
        host = St.t().cpu().numpy()
        return {v: host[:, pcol[v]:pcol[v] + v.dim].copy() for v in self._elimination_ordering}

    def posterior_refine(self, samples=None, n: int = None, steps: int = 100, step_size: float = 1e-2, kernel="variable",
                         sigma=None, standardise: bool = True) -> dict:
        """Posterior samples moved along the score of the joint density p(X, Z), on the device where the sample matrix lies:
        Stein variational gradient descent (nfisam_sample_svgd, nfisam_sample_step: float32 points, float64 arithmetic) --
        phi(x_i) = 1/n sum_j [k(x_j, x_i) grad log p(x_j) + grad_{x_j} k(x_j, x_i)], the descent direction of the statistic
        `posterior_ksd` reports, applied `steps` times with the AdaGrad rule of the original SVGD code.  Not in the reference.

        samples=None draws `n` (default posterior_sample_num) points through the tree walk; otherwise `samples` is refined (as
        `joint_log_pdf` accepts it) and nothing is drawn.  kernel: "variable" one kernel per variable of the elimination
        ordering (each sees its own columns; the fixed point is still p), "joint" one kernel over all columns, None no kernel:
        every point climbs the score alone (see `map_refine`).  standardise: every column's differences are divided by its
        spread over the STARTING points, as in `posterior_ksd`, and a column's step is `step_size` times that spread; otherwise
        the step is `step_size` in every column's own unit.  sigma: the bandwidth in those units, one or (kernel="variable") one
        per variable in ordering order; None = sqrt(block width).  Headings are flagged circular from the variables.  The
        points stay float32: a step below a coordinate's float32 spacing (7.6e-6 at 100 m) is lost.
        -> dict: samples (variable -> [n, dim] float32: valid input to every other evaluation), log_p_before, log_p_after
        ([n] float64: `joint_log_pdf` of the points), steps, kernel, sigma (variable -> bandwidth, one bandwidth for "joint",
        None without kernel), precision (variable -> [dim], scale^2 / sigma^2 as `posterior_ksd` reports it; scale^2 without
        kernel), n.
        A copy of the sample matrix is refined: no solver state changes and refined samples are not fed back; random numbers
        are drawn only when `samples` is None.  Raises RuntimeError when there is no graph / tree yet, NotImplementedError naming
        a factor class without a device code, ValueError for bad points or options -- before anything is launched."""
        from utils import Statistics as ST
        what = "posterior_refine"

        def blocks_of(pts, cols):
            if kernel not in ("variable", "joint", None):
                raise ValueError("%s: kernel must be 'variable', 'joint' or None, got %r" % (what, kernel))
            if kernel == "variable":
                return [pts.cols_of(v) for v in self._elimination_ordering]
            return [cols]

        pts, flags, cols, blocks, scale, step = self._refine_front(what, samples, n, steps, step_size, standardise, blocks_of,
                                                                   sigma if kernel is not None else None)
        pcol, order = pts.pcol, list(self._elimination_ordering)
        work = pts.over(pts.St.clone())                                # never the walk's own tensor
        log_p_before = self._joint_launch(pts)
        res = ST.stein_variational_refine_t(work.St, lambda Xt: self._score_launch(work), blocks, int(steps), step, sigma=sigma
                                            if kernel is not None else None, scale=scale, circular=flags,
                                            kernel=kernel is not None)
        log_p_after = self._joint_launch(work) if res["steps"] else log_p_before
        opt = ST.check_refine_options(pts.total_dim, blocks, sigma if kernel is not None else None)
        sig_col = np.ones(pts.total_dim)
        if kernel is not None:
            for b, s in zip(blocks, opt["sigma"]):
                sig_col[b] = s
        precision = scale * scale / (sig_col * sig_col)
        sig_out = None if kernel is None else float(opt["sigma"][0]) if kernel == "joint" else \
            {v: float(s) for v, s in zip(order, opt["sigma"])}
        return dict(samples=self._samples_of(work.St, pcol), log_p_before=log_p_before.cpu().numpy(),
                    log_p_after=log_p_after.cpu().numpy(), steps=res["steps"], kernel=kernel, sigma=sig_out,
                    precision={v: precision[pcol[v]:pcol[v] + v.dim].copy() for v in order}, n=pts.rows)

    def map_refine(self, samples=None, n: int = None, top: int = 8, steps: int = 200, step_size: float = 1e-2,
                   standardise: bool = True) -> dict:
        """A MAP estimate that is not limited to the best draw: the `top` points of highest joint density log p(X, Z) among
        `samples` (or a fresh posterior draw of `n`) each climb the score alone (`posterior_refine` with kernel=None: the
        AdaGrad steps of nfisam_sample_step), log p is evaluated after every step, and the best iterate of every climber --
        its start included -- is kept on the device.  The result is therefore never below `map_estimate` on the same points.
        standardise: a column's step is `step_size` times its spread over ALL the given points.
        -> dict: map_sample (variable -> [dim] float32), log_p (its joint log density), start_log_p (the best of the input:
        `map_estimate`'s), improved (log_p > start_log_p), climbers ([top] float64: the best log p every climber reached, by
        falling start), steps, top (min(top, n)), n.
        No solver state changes; random numbers are drawn only when `samples` is None.  Raises what `posterior_refine` raises,
        and ValueError for a `top` that is no integer >= 1 -- before anything is launched."""
        from utils import Statistics as ST
        what = "map_refine"

        def blocks_of(pts, cols):
            if isinstance(top, bool) or int(top) != top or int(top) < 1:
                raise ValueError("%s: top must be an integer >= 1, got %r" % (what, top))
            return [cols]

        pts, flags, cols, blocks, scale, step = self._refine_front(what, samples, n, steps, step_size, standardise, blocks_of)
        top = min(int(top), pts.rows)
        log_p = self._joint_launch(pts)
        best_lp, idx = torch.topk(log_p, top)                          # by falling log p
        start_log_p = float(best_lp[0].item())
        work = pts.over(pts.St[:, idx].contiguous())
        best, best_lp = work.St.clone(), best_lp.clone()

        def keep(Xt, t):
            lp = self._joint_launch(work)
            better = lp > best_lp                                      # (False for a NaN: the start stays)
            best_lp.copy_(torch.where(better, lp, best_lp))
            best.copy_(torch.where(better.unsqueeze(0), Xt, best))

        res = ST.stein_variational_refine_t(work.St, lambda Xt: self._score_launch(work), blocks, int(steps), step, scale=scale,
                                            circular=flags, kernel=False, after_step=keep)
        k = int(torch.argmax(best_lp).item())
        row, pcol = best[:, k].cpu().numpy(), pts.pcol
        out_lp = float(best_lp[k].item())
        return dict(map_sample={v: row[pcol[v]:pcol[v] + v.dim].copy() for v in self._elimination_ordering}, log_p=out_lp,
                    start_log_p=start_log_p, improved=bool(out_lp > start_log_p), climbers=best_lp.cpu().numpy(),
                    steps=res["steps"], top=top, n=pts.rows)

    # ---- the samples made exact: Metropolis-adjusted Langevin chains started at the flow's draws, with flow jumps -----------------
    def posterior_mcmc(self, samples=None, n: int = None, steps: int = 200, warmup: int = 100, step_size: float = 0.5,
                       kernel: str = "mala", independence_every: int = 0, frozen=None, standardise: bool = True,
                       seed=None, diagnostics: bool = False) -> dict:
        """Posterior samples whose stationary distribution is the factor graph's own posterior p(X | Z): n parallel
        Metropolis chains, one per sample, on the device where the sample matrix lies (nfisam_sample_propose,
        nfisam_sample_accept between nfisam_factor_graph_log_density and nfisam_factor_graph_score: float32 points, float64
        arithmetic).  Not in the reference.  The chains start at the flow's draws, so every mode the flow found is populated.

        samples=None draws `n` (default posterior_sample_num) points through the tree walk; otherwise the chains start at
        `samples` (as `joint_log_pdf` accepts it) and nothing is drawn.  kernel: "mala" (Langevin proposals along the joint
        score) or "rw" (a random walk: no score launch).  `steps` steps in all, of which the first `warmup` scale one multiplier
        on the step lengths towards the optimal acceptance rate (0.574 / 0.234); after them the step lengths are fixed.
        standardise: a column's step is `step_size` times its spread over the STARTING points (the circular spread for a
        heading; `step_size` itself for a column without spread), else `step_size` in every column's own unit; a heading's step
        is at most Statistics.WRAP_STEP_MAX.  independence_every = k > 0: every k-th step proposes fresh draws of the flow
        (the tree walk, from a generator of its own seeded by `seed` and the step) and accepts them with the weights p / q --
        global jumps between modes; 1 makes every step a jump.  frozen: variables held at their given values (their step is 0):
        the chains then sample p(rest | frozen, Z); not together with jumps, which propose every variable.
        seed: the key of the chains' generator (None: one below 2^62 from numpy's global RNG).
        -> dict: samples (variable -> [n, dim] float32: valid input to every other evaluation), log_p ([n] float64:
        `joint_log_pdf` of them), accept_rate (accepted local proposals / proposed, over chains and steps; None without local
        steps), jump_accept_rate (None without jumps), step_size (variable -> [dim]: the final step lengths), steps, warmup,
        kernel, n, seed.
        diagnostics=True: the state of every chain after every step t >= warmup is folded into streaming accumulators on the
        device (nfisam_chain_record; the history itself is never kept), about the starting points' means, and the result gains
        diagnostics (variable -> dict(mean, rhat, tau, ess, resolved), each [dim]: the mean over chains and recorded states,
        split-R-hat over the 2 n half-chains, the blocking estimate of the integrated autocorrelation time in steps,
        ess = n recorded / tau, and whether the blocking plateau was seen -- resolved False: tau is a LOWER bound and ess an upper
        one, `Statistics.blocking_tau`), rhat_max and ess_min (over the columns that move; NaN if none does) and recorded (the
        number of recorded states, even: of an odd steps - warmup the first post-warm-up state is left out; at least 4 are
        needed).  A frozen variable's rhat, tau and ess are NaN.  The samples are the same bits with and without.
        A copy of the sample matrix is moved: no solver state changes and the result is not fed back.  With `samples` and `seed`
        given no random stream is touched.  Raises RuntimeError when there is no graph / tree yet, NotImplementedError naming a
        factor class without a device code, ValueError for bad points or options -- before anything is launched."""
        from utils import Statistics as ST
        what, every = "posterior_mcmc", independence_every
        count = not isinstance(every, bool) and isinstance(every, (int, np.integer)) and every >= 0
        pts = self._eval_points(what, samples, n, factors=True, log_q=bool(count and every > 0), nonempty=True)
        flags, cols = pts.flags, pts.cols
        order, pcol = list(self._elimination_ordering), pts.pcol
        with _named(what):
            if not count:
                raise ValueError("independence_every must be an integer >= 0, got %r" % (every,))
            if np.ndim(step_size) != 0 or not (np.isfinite(step_size) and step_size > 0):
                raise ValueError("step_size is one positive finite step")
            held = list(frozen) if frozen is not None else []
            if any(v not in pcol or v not in order for v in held):
                raise ValueError("frozen names a variable that is not in the graph")
            if held and every:
                raise ValueError("independence steps propose every variable: not together with frozen variables")
            opt = ST.check_metropolis_options(pts.total_dim, steps, float(step_size), None, kernel, warmup, None, seed)
            if diagnostics:
                ST.check_chain_options(pts.total_dim, opt["steps"], opt["warmup"], {}, least=4)
        scale = self._column_scale(pts, flags, cols, bool(standardise))
        h = np.zeros(pts.total_dim)
        h[cols] = float(step_size)
        if standardise:
            h[scale > 0] = float(step_size) / scale[scale > 0]
        h[flags] = np.minimum(h[flags], ST.WRAP_STEP_MAX)
        for v in held:
            h[pcol[v]:pcol[v] + v.dim] = 0.0
        seed = int(np.random.randint(0, 2 ** 62)) if opt["seed"] is None else opt["seed"]
        work = pts.over(pts.St.clone())                                # never the walk's own tensor

        def draw_t(rows, t):
            tb = pts.table
            K, H, B, L = tb["cfg"]
            gen = torch.Generator(device=pts.device)
            gen.manual_seed((seed ^ (0x9E3779B97F4A7C15 * (t + 1))) & (2 ** 63 - 1))
            Zt = torch.randn(tb["total_dim"], rows, dtype=torch.float32, device=pts.device, generator=gen)
            Y = _nh.posterior_walk_raw(tb["table"], tb["cols"], tb["obs"], tb["total_dim"], rows, tb["max_D"], K, H, B, L,
                                       tb["device"], Zt=Zt).t().contiguous()
            return Y, self._log_q_launch(pts.over(Y))

        record = dict(levels=None, center=None) if diagnostics else None    # (the centres: the starting points' means)
        res = ST.metropolis_refine_t(work.St, lambda Xt: self._joint_launch(pts.over(Xt)),
                                     lambda Xt: self._score_launch(pts.over(Xt)), opt["steps"], h, circular=flags, kernel=kernel,
                                     warmup=opt["warmup"], seed=seed, independence=(int(every), draw_t) if every else None,
                                     log_q_t=(lambda Xt: self._log_q_launch(pts.over(Xt))) if every else None, record=record)
        h_end = res["h"].cpu().numpy()
        local, jump = res["local_steps"], res["jump_steps"]
        out = dict(samples=self._samples_of(work.St, pcol), log_p=res["log_p"].cpu().numpy(),
                   accept_rate=float(res["accepts"].sum().item()) / (local * pts.rows) if local else None,
                   jump_accept_rate=float(res["jump_accepts"].sum().item()) / (jump * pts.rows) if jump else None,
                   step_size={v: h_end[pcol[v]:pcol[v] + v.dim].copy() for v in order}, steps=res["steps"],
                   warmup=res["warmup"], kernel=kernel, n=pts.rows, seed=seed)
        if diagnostics:
            ch = res["chains"]
            moving = cols[h_end[cols] > 0]
            rh, es = ch["rhat"][moving], ch["ess"][moving]
            out.update(diagnostics={v: {k: ch[k][pcol[v]:pcol[v] + v.dim].copy() for k in ("mean", "rhat", "tau", "ess", "resolved")}
                                    for v in order},
                       rhat_max=float(np.max(rh[~np.isnan(rh)])) if np.any(~np.isnan(rh)) else float("nan"),
                       ess_min=float(np.min(es[~np.isnan(es)])) if np.any(~np.isnan(es)) else float("nan"), recorded=ch["T"])
        return out

    # ---- curvature: Hessian-vector products, truncated-Newton MAP ascent, the Laplace approximation at a mode ---------------------
    def _hvp_launch(self, pts: EvalPoints, Vt, score: bool = False):
        """Ht (and, with `score`, Gt) [total_dim, n] float64 on the device: the table and gather lists of `_score_launch`."""
        cache = self._joint_terms(pts.pcol)
        g = cache.get("gather")
        if g is None or g["row_off"].shape[0] != pts.total_dim + 1:
            g = cache["gather"] = _nh.pack_score_gather(cache["terms"], pts.total_dim)
        on = cache.setdefault("gather_dev", {})                        # (the cache is made anew whenever the table grows)
        if pts.rows and (pts.device not in on or on[pts.device]["row_off"].shape[0] != pts.total_dim + 1):
            so, ro, rs = _nh.upload(g["slot_off"], g["row_off"], g["row_slot"], device=pts.device, cached=True)
            on[pts.device] = dict(slot_off=so, row_off=ro, row_slot=rs, n_slots=g["n_slots"])
        # a Newton step is dozens of these calls on one table: the lists stay on the device (Plaza1's are past the staging ring)
        return _nh.factor_graph_hvp_t(cache["terms"], pts.St, Vt, pts.device, gather=on.get(pts.device, g), score=score,
                                      terms_dev=self._joint_terms_dev(cache, pts.device, pts.rows))

    def _hvp_colours(self, pts: EvalPoints):
        """The column classes of `Statistics.probe_colours` for the joint Hessian's sparsity (columns coupled by one factor),
        kept next to the cached table: diag(H) then costs one product per class.  No device."""
        from utils import Statistics as ST
        cache = self._joint_terms(pts.pcol)
        c = cache.get("colours")
        if c is None or c[0] != pts.total_dim:
            slot_off, rows = _nh._slot_rows(cache["terms"])
            ends = list(slot_off[1:]) + [rows.size]
            c = cache["colours"] = (pts.total_dim, ST.probe_colours([rows[a:b] for a, b in zip(slot_off, ends)], pts.total_dim))
        return c[1]

    def joint_hessian_product(self, samples, vectors) -> np.ndarray:
        """H v of the joint density's Hessian H = d^2 log p(X, Z) / dx dx' at n points along one direction per point, on the
        device in float64 at the float32 points (nfisam_factor_graph_hvp: the derivative of `joint_score`'s smooth formula;
        nothing of size total_dim^2 is formed).  Not in the reference.

        samples: as `joint_log_pdf`.  vectors: mapping variable -> [n, dim] (every variable of the ordering), or an
        [n, total_dim] array in the columns of `_post_columns`.  -> np.ndarray [n, total_dim] float64 in those columns.
        Raises what `joint_score` raises, and ValueError for vectors of a wrong shape -- before anything is launched."""
        what = "joint_hessian_product"
        pts = self._eval_points(what, samples, factors=True)
        if isinstance(vectors, dict) or hasattr(vectors, "keys"):
            values, rows = self._check_points(vectors, what, nouns=("vectors lack", "vectors", "ragged vectors", "n"), host=True)
            if rows != pts.rows:
                raise ValueError("%s: vectors have %d rows, the samples %d" % (what, rows, pts.rows))
            V = np.zeros((pts.rows, pts.total_dim))
            for v, a in values.items():
                V[:, pts.pcol[v]:pts.pcol[v] + v.dim] = a
        else:
            V = vectors.detach().cpu().numpy() if torch.is_tensor(vectors) else np.asarray(vectors)
            if V.ndim != 2 or V.shape != (pts.rows, pts.total_dim):
                raise ValueError("%s: vectors must be [n, total_dim] = %s, got %s" % (what, (pts.rows, pts.total_dim), tuple(V.shape)))
        Vt = torch.from_numpy(np.ascontiguousarray(V.T, dtype=np.float64)).to(pts.device)
        return self._hvp_launch(pts, Vt).t().cpu().numpy()

    def map_newton(self, samples=None, n: int = None, top: int = 8, steps: int = 20, cg_iters: int = None, rtol: float = 1e-8,
                   damping: float = 0.0, standardise: bool = True, gtol: float = None, backtracks: int = None) -> dict:
        """A MAP estimate by truncated-Newton ascent: the `top` points of highest joint density log p(X, Z) among `samples` (or
        a fresh posterior draw of `n`) each take up to `steps` Newton steps (`Statistics.newton_refine_t`): the score and the
        Hessian-vector products come from one kernel (nfisam_factor_graph_hvp), the step solves (-H + damping) d = g by
        matrix-free conjugate gradients (at most `cg_iters` products; None: TWICE the number of columns in use), preconditioned
        with diag(H) at the points (one product per class of columns that no factor couples: 6 on the small range graph, 12 on Plaza1), and backtracks
        by halving with one log p launch per trial.  (In exact arithmetic as many products as columns end the solve; in float64
        they do not on a graph that knows one pose to millimetres and a landmark to metres: on the small range problem,
        cond(-H) = 1.5e7 and 2e4 with the diagonal scaled out, 22 products leave the step so inexact that 20 Newton steps are
        needed where 44 products need 4.)  A point only ever moves upwards, so the result is never below `map_estimate`
        on the same points; unlike `map_refine` (which is not changed) the ascent knows when it has arrived: `grad_norm` and
        `converged`.  damping: added to -H's diagonal, in units of 1 / spread^2 of every column with `standardise` (the spreads
        of ALL the given points, `_column_scale`), else in the column's own 1 / unit^2.  gtol, backtracks: None = the defaults
        `newton_refine_t` derives from the float32 floor of the points (1e-3 of the standardised score; 10 halvings).
        -> dict: map_sample (variable -> [dim] float32), log_p (its joint log density), start_log_p (the best of the input:
        `map_estimate`'s), improved, climbers ([top] float64: the log p every climber reached, by falling start), steps (taken),
        grad_norm ([top]: max_c |g_c| spread_c at every climber's point, |g_c| without `standardise`), converged ([top] bool:
        grad_norm <= gtol), negative_curvature ([top] bool: the last step's conjugate gradients met a direction along which
        H is not negative), top (min(top, n)), n.
        No solver state changes; random numbers are drawn only when `samples` is None.  Raises what `joint_score` raises, and
        ValueError naming this method for a bad option -- before anything is launched."""
        from utils import Statistics as ST
        what = "map_newton"
        pts = self._eval_points(what, samples, n, factors=True, nonempty=True)
        flags, cols = pts.flags, pts.cols
        with _named(what):
            if isinstance(top, bool) or int(top) != top or int(top) < 1:
                raise ValueError("top must be an integer >= 1, got %r" % (top,))
            if np.ndim(damping) != 0:
                raise ValueError("damping is one finite value >= 0")
            opt = ST.check_newton_options(pts.total_dim, steps, 2 * int(cols.size) if cg_iters is None else cg_iters, rtol, damping,
                                          ST.NEWTON_GTOL if gtol is None else gtol,
                                          ST.NEWTON_BACKTRACKS if backtracks is None else backtracks, circular=flags)
        scale = self._column_scale(pts, flags, cols, bool(standardise))
        top = min(int(top), pts.rows)
        log_p = self._joint_launch(pts)
        start_lp, idx = torch.topk(log_p, top)                         # by falling log p
        work = pts.over(pts.St[:, idx].contiguous())                   # a copy: never the walk's own tensor
        res = ST.newton_refine_t(work.St, lambda Xt, Vt: self._hvp_launch(work, Vt, score=True), lambda Xt: self._joint_launch(
            work.over(Xt)), opt["steps"], opt["cg_iters"], opt["rtol"], float(damping) * scale * scale, opt["gtol"],
            opt["backtracks"], scale=scale, circular=flags, colours=self._hvp_colours(pts))
        k = int(torch.argmax(res["log_p"]).item())
        row, pcol = work.St[:, k].cpu().numpy(), pts.pcol
        out_lp, start_log_p = float(res["log_p"][k].item()), float(start_lp[0].item())
        return dict(map_sample={v: row[pcol[v]:pcol[v] + v.dim].copy() for v in self._elimination_ordering}, log_p=out_lp,
                    start_log_p=start_log_p, improved=bool(out_lp > start_log_p), climbers=res["log_p"].cpu().numpy(),
                    steps=res["steps"], grad_norm=res["grad_norm"].cpu().numpy(), converged=res["converged"].cpu().numpy(),
                    negative_curvature=res["negative_curvature"].cpu().numpy(), top=top, n=pts.rows)

    def laplace_approximation(self, point=None, variables=None, pairs=None, cg_iters: int = None, rtol: float = 1e-8,
                              max_columns: int = 256, **newton) -> dict:
        """The Gaussian summary of a mode: marginal blocks of the covariance -H^-1 of the Laplace approximation of p(X, Z) at
        `point` (variable -> [dim]; None: `map_newton(**newton)`'s map_sample) -- what a Gaussian SLAM back end reports, and
        the companion of `posterior_modes`: that says where the hypotheses are, this how wide the joint density is at one.
        Every requested column c is one right-hand side e_c: the point is replicated once per requested column and ONE
        batched conjugate-gradient run (`Statistics.conjugate_gradient_t` on nfisam_factor_graph_hvp, preconditioned with
        diag(H) from one product per class of columns that no factor couples; at most `cg_iters` products, None: twice the
        number of columns in use, see `map_newton`) solves -H x = e_c for all of them; nothing of size total_dim^2 is formed.  `residual` says how far
        the run came: on the small range problem as many products as columns leave it at 158 and the blocks 28 % off, twice as
        many reach 8e-9 and the blocks agree with the dense inverse of the host Hessian to 3.5e-11.
        variables: whose [dim, dim] blocks (None: all); pairs: (a, b) tuples whose joint [dim_a + dim_b] blocks, as
        `posterior_summary` takes them.  At most `max_columns` (default 256) columns may be requested: ValueError beyond.
        -> dict: point (variable -> [dim] float32), log_p (at the point), cov (variable -> [dim, dim], symmetrised), pair_cov
        ((a, b) -> [dim_a + dim_b, dim_a + dim_b]), residual (the largest |r| / |b| the runs ended with), negative_curvature
        (bool: some run met a direction along which H is not negative definite -- the point is no strict mode and the blocks
        are then no covariance; reported, not raised).  `log_evidence` is left out: it needs log det(-H), which products
        alone do not give cheaply.
        No solver state changes; random numbers are drawn only for point=None with newton's samples=None.  Raises what
        `joint_score` raises, and ValueError naming this method for a bad point or option -- before anything is launched."""
        from utils import Statistics as ST
        what = "laplace_approximation"
        if point is None:
            point = self.map_newton(**newton)["map_sample"]
        elif newton:
            raise ValueError("%s: %s only apply when the point is found by map_newton (point=None)" % (what, sorted(newton)))
        pts = self._eval_points(what, {v: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).reshape(1, -1)
                                       for v, a in point.items()}, factors=True, nonempty=True)
        known = set(self._elimination_ordering)
        variables = list(self._elimination_ordering) if variables is None else list(variables)
        pairs = [tuple(p) for p in pairs] if pairs is not None else []
        for p in pairs:
            if len(p) != 2:
                raise ValueError("%s: a pair is a tuple (a, b) of two variables" % what)
        for v in variables + [v for p in pairs for v in p]:
            self._need_known(what, v, known)
        want = sorted(set(pts.pcol[v] + c for v in variables + [v for p in pairs for v in p] for c in range(v.dim)))
        with _named(what):
            if isinstance(max_columns, bool) or int(max_columns) != max_columns or int(max_columns) < 1:
                raise ValueError("max_columns must be an integer >= 1, got %r" % (max_columns,))
            if not want:
                raise ValueError("no variable to summarise")
            if len(want) > int(max_columns):
                raise ValueError("%d columns are requested, max_columns is %d" % (len(want), int(max_columns)))
            opt = ST.check_newton_options(pts.total_dim, 0, 2 * int(pts.cols.size) if cg_iters is None else cg_iters, rtol)
        at = {c: j for j, c in enumerate(want)}
        work = pts.over(pts.St[:, :1].expand(pts.total_dim, len(want)).contiguous())
        Bt = torch.zeros(pts.total_dim, len(want), dtype=torch.float64, device=pts.device)
        Bt[torch.as_tensor(want, device=pts.device), torch.arange(len(want), device=pts.device)] = 1.0
        hvp = lambda Vt: self._hvp_launch(work, Vt)
        diag = ST.hessian_diagonal_t(hvp, self._hvp_colours(pts), pts.total_dim, len(want), pts.device)
        cg = ST.conjugate_gradient_t(hvp, Bt, opt["cg_iters"], opt["rtol"], precond=ST.inverse_diagonal(diag, None))
        X = cg["x"].cpu().numpy()

        def block(vs):
            rows = [pts.pcol[v] + c for v in vs for c in range(v.dim)]
            m = X[np.ix_(rows, [at[c] for c in rows])]
            return 0.5 * (m + m.T)

        row = pts.St[:, 0].cpu().numpy()
        return dict(point={v: row[pts.pcol[v]:pts.pcol[v] + v.dim].copy() for v in self._elimination_ordering},
                    log_p=float(self._joint_launch(pts)[0].item()), cov={v: block((v,)) for v in variables},
                    pair_cov={p: block(p) for p in pairs}, residual=float(cg["residual"].max().item()),
                    negative_curvature=bool(cg["negative_curvature"].any().item()))

    # ---- the solver graded against a reference sample set --------------------------------------------------------
    def posterior_mmd(self, reference, samples=None, n: int = None, variables=None, blocks=None, columns: str = "xy",
                      estimator: str = "mmd", sigma=None, standardise: bool = False, joint: bool = True) -> dict:
        """MMD between the posterior and a reference sample set -- how the paper grades NF-iSAM (the reference's
        src/utils/Statistics.py:13-84 and icra_paper/compute_mmd.py: one joint `mmd` per step and the mean over the
        variables of the xy-marginal `mmd`) -- with the joint block, every variable's marginal and any further blocks in ONE
        device launch (nfisam_sample_mmd: float32 points, float64 arithmetic).

        reference: mapping variable -> [m, dim] (numpy or torch): a reference solution, another solver's `sample_posterior`
        output, a LazyPosterior.  samples=None draws `n` (default posterior_sample_num) points through the tree walk and scores
        the device matrix where it lies; otherwise `samples` is what `posterior_log_pdf` accepts and nothing is drawn.
        variables: which to compare and in which order (default: those of the elimination ordering that `reference` holds).
        columns: "xy" the reference's rule, the first two columns of every variable (compute_mmd.py:88-98); "all" adds the
        headings, compared by differences wrapped into [-pi, pi).  standardise: divide each non-circular column's differences
        by the reference set's std of that column (floored at 1e-3).  blocks: further blocks, each a tuple of variables
        (e.g. (pose, landmark)).  estimator, sigma: as `utils.Statistics.mmd_blocks` ("mmd": k_sigma2 = 1; "MMDb" / "MMDu2":
        sigma = sqrt(columns of the block)).
        -> dict: joint (None without `joint`), marginal (variable -> value), marginal_mean (the reference's "marginal mmd"),
        blocks (list), floor = sqrt(1 / m + 1 / n) (the value MMDb takes when no pair of the two sets is within kernel
        reach: a statistic that sits there says nothing), m (reference points), n (posterior points), estimator.
        Raises RuntimeError when there is nothing to grade yet, ValueError for an unknown option, a requested variable that
        the ordering, `reference` or `samples` lack, a wrong width, ragged rows or too few points -- before anything is
        launched."""
        from utils.Statistics import mmd_from_sums
        t = self._mmd_tables("posterior_mmd", reference, samples, n, variables, blocks, columns, estimator, sigma, joint)
        pts, Y, wrap, ycols = t["pts"], t["Y"], t["wrap"], t["ycols"]
        scale = None
        if standardise:
            std = np.maximum(Y.astype(np.float64).std(axis=0), 1e-3)
            scale = np.where(wrap != 0, 1.0, 1.0 / std[ycols])
        _nh.check_mmd_blocks(t["blocks"], t["xcols"], ycols, pts.total_dim, t["width"], scale, t["flags"])
        sums = _nh.mmd_sums_t(pts.St, _nh._columns(Y, pts.device), t["blocks"], t["xcols"], ycols, scale, t["flags"], checked=True)
        return self._mmd_result(t, mmd_from_sums(sums.cpu().numpy(), pts.rows, t["m"], estimator))

    def _mmd_tables(self, what, reference, samples, n, variables, blocks, columns, estimator, sigma, joint) -> dict:
        """What `posterior_mmd` and `posterior_mmd_test` share: the option checks, the two fronts, then what is the MMD's own:
        the estimator's least number of points, the bandwidths (`Statistics.mmd_bandwidths`) and the wrap flags -> dict: pts,
        and of `_reference_front`'s record Y [m, width] float32, m, width, variables; joint, estimator, blocks (MMD_BLOCK_DTYPE),
        xcols, ycols, wrap [entries] uint8, flags (wrap, or None when no entry is an angle).  Nothing is launched."""
        from utils import Statistics as ST
        if estimator not in ST.ESTIMATORS:
            raise ValueError("%s: estimator must be one of %s, got %r" % (what, ST.ESTIMATORS, estimator))
        if columns not in ("xy", "all"):
            raise ValueError("%s: columns must be 'xy' or 'all', got %r" % (what, columns))
        pts = self._eval_points(what, samples, n)
        ref = self._reference_front(what, reference, variables, blocks, joint)
        need = 1 if estimator == "MMDb" else 2
        if ref.m < need or pts.rows < need:
            raise ValueError("%s: %s needs at least %d points in each set (reference %d, posterior %d)"
                             % (what, estimator, need, ref.m, pts.rows))
        pairs = ref.pairs(pts, columns)
        xcols, ycols = (np.concatenate(c).astype(np.int32) for c in zip(*pairs))
        wrap = pts.flags[xcols].astype(np.uint8)
        dims = [p[0].size for p in pairs]
        if sigma is not None and np.size(sigma) == 1:           # (a list of one bandwidth is one bandwidth here)
            sigma = np.asarray(sigma, dtype=np.float64).reshape(())
        sig = ST.mmd_bandwidths(dims, estimator, sigma)
        if sig.size != len(dims) or not np.all(np.isfinite(sig) & (sig > 0)):
            raise ValueError("%s: sigma is one positive bandwidth, or one per block (%d)" % (what, len(dims)))
        return dict(pts=pts, Y=ref.Y, m=ref.m, width=ref.width, variables=ref.variables, joint=joint, estimator=estimator,
                    blocks=_nh.pack_mmd_blocks(dims, sig), xcols=xcols, ycols=ycols, wrap=wrap, flags=wrap if wrap.any() else None)

    def _mmd_result(self, t: dict, val) -> dict:
        """The values `val` [blocks of `_mmd_tables`] under the names `posterior_mmd` returns them by."""
        m, rows, at = t["m"], t["pts"].rows, self._places(val, t["variables"], t["joint"])
        return dict(joint=at["joint"], marginal=at["marginal"], marginal_mean=float(np.mean(list(at["marginal"].values()))),
                    blocks=at["blocks"], floor=float(np.sqrt(1.0 / m + 1.0 / rows)), m=m, n=rows, estimator=t["estimator"])

    def posterior_mmd_test(self, reference, samples=None, n: int = None, variables=None, blocks=None, columns: str = "xy",
                           estimator: str = "mmd", sigma=None, standardise: bool = False, joint: bool = True,
                           permutations: int = 999, seed=0, alpha: float = 0.05) -> dict:
        """`posterior_mmd` with what its numbers are worth: the permutation test of H0 "the posterior samples and the
        reference set come from one law", for the joint block, every variable's marginal and every further block.  The two
        sets are pooled and relabelled `permutations` times (`Statistics.permutation_labels(n, m, permutations, seed)`: the
        posterior points are the first set); a p-value is how often the relabelled statistic reaches the observed one --
        exact under exchangeability, with ONE reference set.  All blocks and permutations in one device launch per chunk of
        permutations (nfisam_sample_mmd_perm: every Gram value once for 256 permutations); the observed values come from
        `posterior_mmd`'s own launch.

        Arguments as `posterior_mmd`, except: standardise divides each non-circular column's differences by the std of that
        column over the POOLED set (floored at 1e-3) -- a scale taken from one of the sets would change with the labels and
        break the exchangeability the test rests on; without it the values are `posterior_mmd`'s bit for bit.
        permutations >= 1; alpha in (0, 1): the level of `threshold` and `rejected`.
        -> what `posterior_mmd` returns, and p_value {joint (None without `joint`), marginal: {variable: p}, blocks: [...]},
        p = (1 + #{null >= observed}) / (1 + permutations) ("mmd" is compared on its MMDu2 values, so a NaN never enters);
        marginal_p_holm {variable: Holm-adjusted p over the variables}; rejected [variables with adjusted p <= alpha];
        threshold (the same three places: the (1 - alpha) quantile of the null, the observed value included);
        permutations, seed, alpha.  Raises what `posterior_mmd` raises and ValueError for permutations < 1 or a bad alpha --
        before anything is launched."""
        from utils import Statistics as ST
        what = "posterior_mmd_test"
        permutations = int(permutations)
        if permutations < 1:
            raise ValueError("%s: permutations must be >= 1, got %d" % (what, permutations))
        if not 0.0 < alpha < 1.0:
            raise ValueError("%s: alpha must lie in (0, 1), got %r" % (what, alpha))
        t = self._mmd_tables(what, reference, samples, n, variables, blocks, columns, estimator, sigma, joint)
        pts, Y, wrap, xcols, ycols, m = t["pts"], t["Y"], t["wrap"], t["xcols"], t["ycols"], t["m"]
        rows, variables = pts.rows, t["variables"]
        labels = ST.permutation_labels(rows, m, permutations, seed)
        scale = None
        if standardise:                                             # the pooled spread: the same under every relabelling
            X = pts.St[torch.from_numpy(xcols.astype(np.int64)).to(pts.device)].cpu().numpy().astype(np.float64)
            std = np.maximum(np.concatenate([X, Y.astype(np.float64)[:, ycols].T], axis=1).std(axis=1), 1e-3)
            scale = np.where(wrap != 0, 1.0, 1.0 / std)
        _nh.check_mmd_blocks(t["blocks"], xcols, ycols, pts.total_dim, t["width"], scale, t["flags"])
        Yt = _nh._columns(Y, pts.device)
        obs = _nh.mmd_sums_t(pts.St, Yt, t["blocks"], xcols, ycols, scale, t["flags"], checked=True)
        null = _nh.mmd_perm_sums_t(pts.St, Yt, t["blocks"], xcols, ycols, labels, scale, t["flags"], checked=True)
        res = ST.permutation_test_from_sums(obs.cpu().numpy(), null.cpu().numpy(), rows, m, estimator, alpha)
        out = self._mmd_result(t, res["statistic"])
        k0 = 1 if joint else 0
        holm = ST.holm_adjust(res["p_value"][k0:k0 + len(variables)])
        out.update(p_value=self._places(res["p_value"], variables, joint), threshold=self._places(res["threshold"], variables, joint),
                   marginal_p_holm={v: float(holm[i]) for i, v in enumerate(variables)},
                   rejected=[v for i, v in enumerate(variables) if holm[i] <= alpha],
                   permutations=permutations, seed=seed, alpha=float(alpha))
        return out

    def posterior_transport(self, reference, samples=None, n: int = None, variables=None, blocks=None, columns: str = "xy",
                            p: int = 2, directions: int = 64, seed: int = 0, joint: bool = True, axes: bool = True) -> dict:
        """How far the posterior must be moved to become a reference sample set, in the variables' own units: the sliced
        Wasserstein distance W_p of the joint block, of every variable's marginal and of any further blocks, every (block,
        direction) slice in ONE device launch (nfisam_sample_sliced_transport: float32 points, float64 keys).  Where
        `posterior_mmd` has no unit, needs a bandwidth and sits at its floor once the sets are out of kernel reach, this
        number keeps growing with the separation, sees a missing mode as mass times distance and needs no bandwidth.

        reference, samples, n, variables, blocks, columns, joint: as `posterior_mmd`, with the same front and the same
        handling of the reference; columns="all" adds the headings by the chord embedding (a heading enters as its cosine
        and its sine: continuous across +-pi, the radian difference for small differences).  p: 1 or 2.  directions: per
        block, `Statistics.transport_directions(entries of the block, directions, seed)` -- they depend on (seed, entries)
        alone, so a variable's marginal is the same number in any table.  axes: also the exact 1-D W_p of every entry of every
        variable (basis-vector directions in the same launch).  At most 8192 points in either set.
        -> dict: joint (None without `joint`), marginal (variable -> distance), marginal_mean, marginal_max, max_sliced
        (variable -> max-sliced distance, and "joint"), axes (variable -> per-entry exact 1-D distances; None without
        `axes`), blocks (list), m (reference points), n (posterior points), p, directions.
        Raises RuntimeError when there is nothing to grade yet, ValueError for an unknown option, a requested variable that
        the ordering, `reference` or `samples` lack, a wrong width, ragged rows, an empty set or one of more than 8192
        points -- before anything is launched."""
        from utils import Statistics as ST
        what = "posterior_transport"
        with _named(what):
            ST.check_transport_options(p, directions, seed)
        if columns not in ("xy", "all"):
            raise ValueError("%s: columns must be 'xy' or 'all', got %r" % (what, columns))
        t = self._transport_tables(what, reference, samples, n, variables, blocks, columns, int(directions), int(seed), joint, axes)
        pts, tab, variables = t["pts"], t["tab"], t["variables"]
        _nh.check_transport_blocks(tab["blocks"], tab["xcols"], tab["ycols"], pts.total_dim, t["width"], tab["dirs"], tab["kind"])
        out = _nh.sliced_transport_t(pts.St, _nh._columns(t["Y"], pts.device), tab["blocks"], tab["xcols"], tab["ycols"], tab["dirs"],
                                     p, tab["kind"], None, checked=True)
        res = ST.transport_result(out.cpu().numpy(), tab, p)
        dist, top = self._places(res["distance"], variables, joint), self._places(res["max_sliced"], variables, joint)
        marginal = dist["marginal"]
        return dict(joint=dist["joint"], marginal=marginal, marginal_mean=float(np.mean(list(marginal.values()))),
                    marginal_max=float(np.max(list(marginal.values()))),
                    max_sliced=dict(top["marginal"], joint=top["joint"]) if joint else top["marginal"],
                    axes=self._places(res["axis"], variables, joint, item=lambda a: a)["marginal"] if axes else None,
                    blocks=dist["blocks"], m=t["m"], n=pts.rows, p=int(p), directions=int(directions))

    def _transport_tables(self, what, reference, samples, n, variables, blocks, columns, directions, seed, joint, axes) -> dict:
        """The two fronts of `posterior_transport` (those of `posterior_mmd`), then what is the transport's own: 1..8192 points
        in either set, the directions, and the exact per-entry distances (`axes`) of every variable's own block -> dict: pts,
        of `_reference_front`'s record Y [m, width] float32, m, width, variables; tab (`Statistics.transport_tables` over
        `Statistics.transport_entries`: a heading enters as two entries).  Nothing is launched."""
        from utils import Statistics as ST
        pts = self._eval_points(what, samples, n)
        ref = self._reference_front(what, reference, variables, blocks, joint)
        for name, k in (("reference", ref.m), ("posterior", pts.rows)):
            if not 1 <= k <= _nh.TRANSPORT_MAX_N:
                raise ValueError("%s: the %s set has %d points; a set holds 1..%d" % (what, name, k, _nh.TRANSPORT_MAX_N))
        k0 = 1 if joint else 0
        flags = [bool(axes) and k0 <= b < k0 + len(ref.variables) for b in range(len(ref.table))]
        with _named(what):
            tab = ST.transport_tables(ST.transport_entries(ref.pairs(pts, columns), pts.flags), directions, seed, flags)
        return dict(pts=pts, Y=ref.Y, m=ref.m, width=ref.width, variables=ref.variables, tab=tab)

    # ---- what posterior_summary and posterior_modes share: arguments, block table, the weights ------------------------------
    def _summary_front(self, what, samples, n, variables, pairs, weights):
        """The 'importance' spelling, the front, then the checks of the block arguments -> (pts, importance, variables, pairs)."""
        importance = isinstance(weights, str)
        if importance and weights != "importance":
            raise ValueError("%s: weights is None, an [n] array or 'importance', got %r" % (what, weights))
        pts = self._eval_points(what, samples, n, factors=importance, log_q=importance, nonempty=True)
        known = set(self._elimination_ordering)
        variables = list(self._elimination_ordering) if variables is None else list(variables)
        pairs = [tuple(p) for p in pairs] if pairs is not None else []
        if not variables:
            raise ValueError("%s: no variable to summarise" % what)
        for p in pairs:
            if len(p) != 2:
                raise ValueError("%s: a pair is a tuple (a, b) of two variables" % what)
        for v in variables + [v for p in pairs for v in p]:
            self._need_known(what, v, known)
        for a, b in pairs:
            if a.dim + b.dim > _nh.MOMENTS_MAX_D:
                raise ValueError("%s: the pair (%s, %s) is %d columns wide; a block holds at most %d"
                                 % (what, a.name, b.name, a.dim + b.dim, _nh.MOMENTS_MAX_D))
        return pts, importance, variables, pairs

    @staticmethod
    def _summary_weights(what, weights, importance, rows):
        """-> the checked [rows] float64 host weights (a device tensor is brought over); None without weights, for "importance"."""
        if weights is None or importance:
            return None
        with _named(what):
            return _nh._check_weights(weights.detach().cpu().numpy() if torch.is_tensor(weights) else weights, rows)

    @staticmethod
    def _summary_table(pts: EvalPoints, variables, pairs):
        """-> (table, cols, circ): every variable, then every pair; entry = one column of the sample matrix."""
        table = [(v,) for v in variables] + pairs
        cols = np.concatenate([pts.cols_of(v) for blk in table for v in blk]).astype(np.int32)
        return table, cols, pts.flags[cols].astype(np.uint8)

    def _weights(self, what, pts: EvalPoints, importance, w_host):
        """-> (weights: None, the host array or, for "importance", exp(log w - max) on the device; ess)."""
        if importance:
            log_p, log_q = self._log_p_q(pts)
            log_w = log_p - log_q.to(torch.float64)
            w_dev = torch.exp(log_w - log_w.max())
            ess = float((w_dev.sum() ** 2 / (w_dev * w_dev).sum()).item())
            if not np.isfinite(ess):
                raise ValueError("%s: the importance weights are not finite" % what)
            return w_dev, ess
        if w_host is not None:
            return w_host, float(w_host.sum() ** 2 / (w_host * w_host).sum())
        return None, float(pts.rows)

    # ---- what the posterior says: point estimates, spreads, intervals ---------------------------------------------
    def posterior_summary(self, samples=None, n: int = None, variables=None, pairs=None, weights=None, quantiles=None,
                          truth=None) -> dict:
        """Means, covariances, heading concentrations and quantiles of the posterior, computed on the device from the sample
        matrix the tree walk left there -- brought into the column-major layout the kernels read on the device, once, and
        never copied to the host -- (nfisam_sample_moments / nfisam_sample_quantiles: float32 points, float64
        arithmetic, every variable and pair in one call) -- what the reference does on the host with `sample_mean` and numpy
        after copying the whole matrix out (src/utils/Statistics.py:142-214 and its run scripts).

        samples=None draws `n` (default posterior_sample_num) points through the tree walk; otherwise `samples` is what
        `posterior_log_pdf` accepts, nothing is drawn and no solver state is touched.  variables: which to summarise (default:
        the elimination ordering).  pairs: (a, b) tuples, each summarised as ONE joint block of a.dim + b.dim <= 16 columns.
        weights: None, an [n] array of non-negative weights, or "importance": the self-normalised importance weights
        exp(log p - log q - max) of the same matrix (the log w of `posterior_diagnostics`), kept on the device.  quantiles: a
        list of probabilities (not together with weights; n <= 16384).  truth: variable -> [dim] ground truth.
        -> dict: mean (variable -> [dim]; a heading's is the circular mean in [-pi, pi)), cov (variable -> [dim, dim]: population
        form; a heading's deviations are wrapped about its circular mean), resultant (variable -> mean resultant length of its
        heading, for variables that have one), pair_cov ((a, b) -> matrix), quantiles (variable -> [n_probs, dim], None when not
        asked for; a heading's are NOT wrapped back into [-pi, pi) so that an interval's ends stay ordered), n, ess
        ((sum w)^2 / sum w^2; n without weights), and with `truth`, over the summarised variables that `truth` holds:
        translation_rmse (utils.Statistics.translation_distance of the means), translation_error (variable -> its term, the
        squared xy distance), geodesic (utils.Statistics.geodesic_distance).
        Raises RuntimeError when there is nothing to summarise yet; ValueError for an unknown variable, a wrong width, ragged
        rows, bad weights or probabilities, quantiles with weights or with more than 16384 points, a pair wider than 16 columns
        -- before anything is launched."""
        from utils import Statistics as ST
        what = "posterior_summary"
        pts, importance, variables, pairs = self._summary_front(what, samples, n, variables, pairs, weights)
        rows = pts.rows
        probs = None
        if quantiles is not None:
            if weights is not None:
                raise ValueError("%s: quantiles are unweighted; ask for them without weights" % what)
            probs = np.asarray(quantiles, dtype=np.float64).reshape(-1)
            if probs.size < 1 or not np.all((probs >= 0.0) & (probs <= 1.0)):
                raise ValueError("%s: quantiles is a non-empty list of probabilities in [0, 1]" % what)
            if rows > _nh.QUANTILE_MAX_N:
                raise ValueError("%s: quantiles take at most %d points, got %d" % (what, _nh.QUANTILE_MAX_N, rows))
        w_host = self._summary_weights(what, weights, importance, rows)
        graded = []
        if truth is not None:
            graded = [v for v in variables if v in truth]
            if not graded:
                raise ValueError("%s: truth holds none of the summarised variables" % what)
            for v in graded:
                if np.ndim(truth[v]) != 1 or len(truth[v]) != v.dim:
                    raise ValueError("%s: truth of %s must be [%d], got shape %s" % (what, v.name, v.dim, np.shape(truth[v])))

        # the table: every variable, then every pair; entry = one column of the sample matrix
        table, cols, circ = self._summary_table(pts, variables, pairs)
        blocks = _nh.pack_moment_blocks([sum(v.dim for v in blk) for blk in table])
        _nh.check_moment_blocks(blocks, cols, pts.total_dim, circ)
        flags = circ if circ.any() else None
        w_dev, ess = self._weights(what, pts, importance, w_host)
        mean_d, res_d, cov_d = _nh.sample_moments_t(pts.St, blocks, cols, flags, w_dev, checked=True)
        q = None
        if probs is not None:
            nq = sum(v.dim for v in variables)
            q = _nh.sample_quantiles_t(pts.St, cols[:nq], probs, None if flags is None else circ[:nq], mean_d[:nq], checked=True)
            q = q.cpu().numpy()
        mean, res, cov = mean_d.cpu().numpy(), res_d.cpu().numpy(), cov_d.cpu().numpy()
        out = dict(mean={}, cov={}, resultant={}, pair_cov={}, quantiles=None if q is None else {}, n=rows, ess=ess)
        for blk, row in zip(table, blocks):
            o, d, c = int(row["col_off"]), int(row["d"]), int(row["cov_off"])
            m = cov[c:c + d * d].reshape(d, d).copy()
            if len(blk) == 2:
                out["pair_cov"][blk] = m
                continue
            v = blk[0]
            out["mean"][v], out["cov"][v] = mean[o:o + d].copy(), m
            heading = [k for k, f in enumerate(v.circular_dim_list) if f]
            if heading:
                out["resultant"][v] = float(res[o + heading[0]]) if len(heading) == 1 else res[o:o + d][heading].copy()
            if q is not None:
                out["quantiles"][v] = q[o:o + d].T.copy()
        if truth is not None:
            est = {v: out["mean"][v] for v in graded}
            ref = {v: np.asarray(truth[v], dtype=np.float64) for v in graded}
            out["translation_rmse"] = float(ST.translation_distance(est, ref))
            out["translation_error"] = {v: float(e) for v, e in ST.translation_terms(est, ref).items()}
            out["geodesic"] = float(ST.geodesic_distance(est, ref))
        return out

    # ---- which hypotheses the posterior holds: modes, their masses, who belongs to which -----------------------------
    def posterior_modes(self, samples=None, n: int = None, variables=None, pairs=None, weights=None, sigma=None, tol=1e-7,
                        merge=1e-2, max_iters=500, max_modes=16) -> dict:
        """The modes of every variable's marginal posterior, found on the device from the sample matrix the tree walk left
        there (nfisam_sample_modes: from every sample a mean-shift ascent on the Gaussian kernel density estimate of the
        variable's own samples, then a deterministic merge of the converged points; float32 points, float64 arithmetic, every
        variable and pair in one call).  Where `posterior_summary` reports one mean between the hypotheses of a bimodal
        variable, this reports each hypothesis, its mass and its members.

        samples, n, variables, pairs and weights are those of `posterior_summary` (a pair (a, b) is ONE joint block of
        a.dim + b.dim <= 16 columns; weights: None, an [n] array or "importance").  Columns are standardised by their
        (weighted) spread -- the circular standard deviation for a heading, whose differences are wrapped: a mode may sit across
        the +-pi seam -- and a column without spread is ignored.  sigma: one bandwidth or one per block (variables, then pairs)
        in those units; None: Scott's rule ess^(-1 / (dim + 4)).  tol, merge: in sigmas; max_modes <= 32.
        Every bump of the density estimate is a mode: with Scott's rule a near-Gaussian marginal of some hundred samples has
        small ones in its tails, and ascents there can run into max_iters.  Read `mass` before counting hypotheses and
        `not_converged` before trusting a position; a larger `sigma` smooths the bumps away.
        -> dict: modes (variable -> list of {position [dim], mass, density}, by falling density), pair_modes ((a, b) -> list),
        labels (variable -> device int32 [n]: the mode of every sample, -1 for one left over when max_modes was reached), n,
        ess, sigma (variable or pair -> the bandwidth used), not_converged (variable or pair -> ascents that stopped on
        max_iters), unlabelled (variable or pair -> count).
        It changes no solver state and draws random numbers only when `samples` is None.  Raises what `posterior_summary`
        raises, and ValueError for a bad sigma, tol, merge, max_iters or max_modes -- before anything is launched."""
        from utils import Statistics as ST
        what = "posterior_modes"
        pts, importance, variables, pairs = self._summary_front(what, samples, n, variables, pairs, weights)
        with _named(what):
            sigma, _ = ST.check_mode_options(len(variables) + len(pairs), 1, sigma, None, tol, merge, max_iters, max_modes)
        w_host = self._summary_weights(what, weights, importance, pts.rows)
        table, cols, _ = self._summary_table(pts, variables, pairs)
        w_dev, ess = self._weights(what, pts, importance, w_host)
        blocks, at = [], 0
        for blk in table:
            d = sum(v.dim for v in blk)
            blocks.append(cols[at:at + d])
            at += d
        res = ST.sample_modes_t(pts.St, blocks, circular=pts.flags, weights=w_dev, sigma=sigma, tol=tol, merge=merge,
                                max_iters=max_iters, max_modes=max_modes, checked=True)
        out = dict(modes={}, pair_modes={}, labels={}, n=pts.rows, ess=ess, sigma={}, not_converged={}, unlabelled={})
        for b, blk in enumerate(table):
            key = blk if len(blk) == 2 else blk[0]
            out["pair_modes" if len(blk) == 2 else "modes"][key] = res["modes"][b]
            if len(blk) == 1:
                out["labels"][key] = res["labels"][b]
            out["sigma"][key] = float(res["sigma"][b])
            out["not_converged"][key] = int(res["iterations"]["not_converged"][b])
            out["unlabelled"][key] = int(res["unlabelled"][b])
        return out

    # ---- how uncertain a variable is and how strongly two are coupled: entropies by k nearest neighbours -------------
    def posterior_information(self, samples=None, n: int = None, variables=None, pairs=None, k: int = 4, standardise: bool = True,
                              reference=None) -> dict:
        """The differential entropy of every variable's marginal posterior and the mutual information of pairs of variables,
        in nats, from the sample matrix the tree walk left on the device: the k nearest neighbours of every sample within
        every block in one launch (nfisam_sample_knn / nfisam_sample_ball_count: float32 points, float64 arithmetic, max
        norm), the Kozachenko-Leonenko and Kraskov-Stoegbauer-Grassberger formulas on the host
        (utils.Statistics.knn_entropy_t, knn_mutual_information_t).  1/2 log det(2 pi e Sigma) from `posterior_summary`
        overstates the uncertainty of a ring or of two modes by nats; the entropy here does not, and the difference of the
        two -- the negentropy -- says how far from Gaussian a marginal is.

        samples, n, variables and pairs are those of `posterior_summary` (samples=None draws `n`, default
        posterior_sample_num, points and works on the device matrix where it lies).  k: 1..16 neighbours (more than k
        samples are needed).  standardise: distances in columns divided by their spread (the circular standard deviation of
        a heading, whose differences are wrapped), the entropy brought back to the original units; False: raw columns.
        reference: mapping variable -> [m, dim] samples of another solution: adds `divergence`, the k-nearest-neighbour
        estimate of KL(posterior || reference) of every variable that `reference` holds, over all its columns.
        A joint block (a pair for the mutual information) wider than 16 columns is refused: the estimators' bias grows with
        the dimension, and a k-nearest-neighbour entropy in hundreds of dimensions means nothing at n around 2000 -- which is
        why there is no joint entropy of the whole graph here.
        -> dict: entropy (variable -> nats; -inf for a variable with a column without spread, NaN when no sample could be
        used), gaussian_entropy (variable -> 1/2 log det(2 pi e Sigma), Sigma the covariance `posterior_summary` reports for
        the same points), negentropy (variable -> gaussian_entropy - entropy), mutual_information ((u, v) -> nats, for the
        listed pairs; about 0, possibly slightly negative, for independent variables), divergence (variable -> nats; only with
        `reference`), n, k, zeros (variable or pair -> samples left out because their k-th neighbour is at distance 0:
        duplicates).
        It consumes no random numbers (a draw apart), changes nothing in the solver, and raises what `posterior_summary`
        raises, and ValueError for a bad k, too few samples, or a reference that lacks rows or has the wrong width -- before
        anything is launched."""
        from utils import Statistics as ST
        what = "posterior_information"
        pts, _, variables, pairs = self._summary_front(what, samples, n, variables, pairs, None)
        rows = pts.rows
        with _named(what):
            ST.check_knn_options(pts.total_dim, k, "max", None, m=rows)
        if reference is not None:
            graded = [v for v in variables if v in reference]
            if not graded:
                raise ValueError("%s: the reference holds none of the variables" % what)
            ref = self._reference_layout(what, reference, graded)
            if ref.m < int(k):
                raise ValueError("%s: the reference's %d points hold no %d-th neighbour" % (what, ref.m, int(k)))
        flags, cols_of = pts.flags, pts.cols_of
        scale = None if standardise else np.ones(pts.total_dim)
        St = pts.St

        ent = ST.knn_entropy_t(St, [cols_of(v) for v in variables], k, flags, scale, "max", checked=True)
        table, cols, circ = self._summary_table(pts, variables, [])
        blocks = _nh.pack_moment_blocks([v.dim for v in variables])
        _, _, cov_d = _nh.sample_moments_t(St, blocks, cols, circ if circ.any() else None, None, checked=True)
        cov = cov_d.cpu().numpy()
        out = dict(entropy={}, gaussian_entropy={}, negentropy={}, mutual_information={}, n=rows, k=int(k), zeros={})
        for b, (v, row) in enumerate(zip(variables, blocks)):
            d, c = int(row["d"]), int(row["cov_off"])
            sign, logdet = np.linalg.slogdet(cov[c:c + d * d].reshape(d, d))
            gauss = 0.5 * (d * np.log(2.0 * np.pi * np.e) + logdet) if sign > 0 else float("-inf")
            out["entropy"][v], out["gaussian_entropy"][v] = float(ent["entropy"][b]), float(gauss)
            with np.errstate(invalid="ignore"):
                out["negentropy"][v] = float(np.float64(gauss) - ent["entropy"][b])
            out["zeros"][v] = int(ent["zeros"][b])
        if pairs:
            mi = ST.knn_mutual_information_t(St, [(cols_of(a), cols_of(b)) for a, b in pairs], k, flags, scale, checked=True)
            for p, pair in enumerate(pairs):
                out["mutual_information"][pair], out["zeros"][pair] = float(mi["mi"][p]), int(mi["zeros"][p])
        if reference is not None:
            div = ST.knn_divergence_t(St, _nh._columns(ref.Y, pts.device), ref.pairs(pts), k, flags, scale, "max", checked=True)
            out["divergence"] = {v: float(div["divergence"][b]) for b, v in enumerate(graded)}
        return out

    # ---- the marginal density itself: curves, maps, the density at the truth -------------------------------------------
    def posterior_marginal_density(self, samples=None, n: int = None, variables=None, pairs=None, weights=None, bandwidth="scott",
                                   curves=None, maps=None, at=None, truth=None) -> dict:
        """The marginal posterior density of variables at points the caller chooses: a Gaussian kernel density estimate of
        the sample matrix the tree walk left on the device, evaluated there in logs (nfisam_sample_density: float32 points,
        float64 arithmetic, a full bandwidth matrix per block, every block of a kind of query in one launch) -- what the
        reference's figures compute on the host with scipy.stats.gaussian_kde per coordinate (example/slam/*/kde_plot_grid.py),
        and what a calibration score needs: RMSE says where the estimate is, not whether its uncertainty is right.

        samples, n, variables, pairs and weights are those of `posterior_summary` (a pair (a, b) is ONE joint block, here of
        at most 6 columns).  bandwidth: "scott", "silverman", a positive factor (scipy's rules, utils.Statistics.
        density_bandwidth) or "loo", the factor with the largest mean leave-one-out log density -- on a ring or on two
        hypotheses Scott's rule is several times too wide.  At least one of:
          curves=g      every coordinate of every variable alone on g points from its min - 3 h to its max + 3 h (a heading:
                        [-pi, pi)) -> curves[v][c] = {x [g], density [g], h}: the reference's kde_plot_grid at kde_pts = g;
          maps=(gx, gy) the xy block of every variable of two or more columns -> maps[v] = {x [gx], y [gy], density [gy, gx], H};
          at            mapping variable or pair -> [q, dim] points, the whole block evaluated (heading included)
                        -> log_density[key] [q];
          truth         mapping variable -> [dim] -> nlpd[v] = -log density at the truth, hpd_level[v] (the credible level of
                        the smallest highest-density region that holds it: utils.Statistics.hpd_level, one more launch with
                        the samples as queries), mean_nlpd, coverage {0.5, 0.9, 0.95 -> the share of graded variables whose
                        hpd_level is at most that level}.
        One launch per kind of query.  -> dict with those keys (None for a kind not asked for), bandwidth (variable or pair ->
        {factor, H}), n, ess.  It changes no solver state and draws only when `samples` is None.  Raises what
        `posterior_summary` raises, and ValueError for a bad bandwidth, grid, point set or truth, or a pair wider than 6
        columns -- before anything is launched; for a column without spread or a heading whose kernel would be wider than
        pi / 3 -- before any density is evaluated."""
        from utils import Statistics as ST
        what = "posterior_marginal_density"
        pts, importance, variables, pairs = self._summary_front(what, samples, n, variables, pairs, weights)
        rows = pts.rows
        for a, b in pairs:
            if a.dim + b.dim > _nh.DENSITY_MAX_D:
                raise ValueError("%s: the pair (%s, %s) is %d columns wide; a density block holds at most %d"
                                 % (what, a.name, b.name, a.dim + b.dim, _nh.DENSITY_MAX_D))
        for v in variables:
            if v.dim > _nh.DENSITY_MAX_D:
                raise ValueError("%s: %s is %d columns wide; a density block holds at most %d" % (what, v.name, v.dim, _nh.DENSITY_MAX_D))
        if curves is None and maps is None and at is None and truth is None:
            raise ValueError("%s: ask for at least one of curves, maps, at or truth" % what)
        with _named(what):
            ST.check_density_options(bandwidth, rows)
        if curves is not None and (isinstance(curves, bool) or int(curves) != curves or int(curves) < 2):
            raise ValueError("%s: curves is the number of grid points, an integer >= 2, got %r" % (what, curves))
        map_vars = []
        if maps is not None:
            if np.ndim(maps) != 1 or len(maps) != 2 or any(isinstance(g, bool) or int(g) != g or int(g) < 2 for g in maps):
                raise ValueError("%s: maps is (gx, gy), two integers >= 2, got %r" % (what, maps))
            map_vars = [v for v in variables if v.dim >= 2]
            if not map_vars:
                raise ValueError("%s: no variable has an xy block to map" % what)
        at_keys, at_pts = [], []
        if at is not None:
            for key, p in at.items():
                blk = tuple(key) if isinstance(key, (tuple, list)) else (key,)
                if (len(blk) == 2 and blk not in pairs) or (len(blk) == 1 and blk[0] not in variables) or len(blk) > 2:
                    raise ValueError("%s: at names %s, which is not among the variables and pairs of this call"
                                     % (what, "(%s)" % ", ".join(getattr(v, "name", str(v)) for v in blk)))
                p = np.asarray(p.detach().cpu().numpy() if torch.is_tensor(p) else p, dtype=np.float64)
                d = sum(v.dim for v in blk)
                if p.ndim != 2 or p.shape[1] != d or p.shape[0] < 1:
                    raise ValueError("%s: at[%s] must be [q >= 1, %d], got %s" % (what, "/".join(v.name for v in blk), d, p.shape))
                at_keys.append(blk), at_pts.append(p)
            if not at_keys:
                raise ValueError("%s: at is empty" % what)
        graded = []
        if truth is not None:
            graded = [v for v in variables if v in truth]
            if not graded:
                raise ValueError("%s: truth holds none of the variables" % what)
            for v in graded:
                if np.ndim(truth[v]) != 1 or len(truth[v]) != v.dim or not np.all(np.isfinite(np.asarray(truth[v], dtype=np.float64))):
                    raise ValueError("%s: truth of %s must be [%d] finite values, got shape %s" % (what, v.name, v.dim, np.shape(truth[v])))
        w_host = self._summary_weights(what, weights, importance, rows)
        table, cols, _ = self._summary_table(pts, variables, pairs)
        w_dev, ess = self._weights(what, pts, importance, w_host)
        flags = pts.flags

        # every block whose bandwidth is needed: variables and pairs, then the curves' coordinates, then the maps' xy blocks
        blocks, at_col = [], 0
        for blk in table:
            d = sum(v.dim for v in blk)
            blocks.append(cols[at_col:at_col + d].astype(np.int64))
            at_col += d
        index = {blk: b for b, blk in enumerate(table)}
        curve_of, map_of = {}, {}
        if curves is not None:
            for v in variables:
                for c in range(v.dim):
                    curve_of[(v, c)] = len(blocks)
                    blocks.append(np.array([pts.pcol[v] + c], dtype=np.int64))
        for v in map_vars:
            map_of[v] = len(blocks)
            blocks.append(np.array([pts.pcol[v], pts.pcol[v] + 1], dtype=np.int64))
        St = pts.St
        device = St.device
        bw = ST.density_bandwidths_t(St, blocks, flags, w_dev, bandwidth)
        log_w, log_w_sum = _nh.density_log_weights(w_dev, rows, device, checked=True)

        def launch(Qt, which, qcols, want_density=False):
            """One launch: blocks `which` (indices into `blocks`) against the queries Qt, block k reading rows qcols[k] of it."""
            xc = np.concatenate([blocks[b] for b in which])
            wrap = flags[xc].astype(np.uint8)
            wrap = wrap if wrap.any() else None
            tab = _nh.pack_density_blocks([blocks[b].size for b in which], [bw["W"][b] for b in which])
            qc = np.concatenate(qcols)
            _nh.check_density_blocks(tab, qc, xc, int(Qt.shape[0]), pts.total_dim, wrap)
            return _nh.sample_density_t(Qt, St, tab, qc, xc, wrap, log_w, False, want_density, checked=True, log_w_sum=log_w_sum)

        out = dict(curves=None, maps=None, log_density=None, n=rows, ess=ess,
                   bandwidth={(blk if len(blk) == 2 else blk[0]): dict(factor=float(bw["factor"][b]), H=bw["H"][b].copy())
                              for blk, b in index.items()})
        if curves is not None or map_vars:
            used = np.unique(np.concatenate([blocks[b] for b in list(curve_of.values()) + list(map_of.values())]))
            lo_d, hi_d = St[used].min(dim=1).values.double().cpu().numpy(), St[used].max(dim=1).values.double().cpu().numpy()
            lo, hi = dict(zip(used.tolist(), lo_d)), dict(zip(used.tolist(), hi_d))

        def axis(col, h, g):
            if flags[col]:
                return np.linspace(-np.pi, np.pi, g, endpoint=False).astype(np.float32)
            return np.linspace(lo[col] - 3.0 * h, hi[col] + 3.0 * h, g).astype(np.float32)

        if curves is not None:
            g = int(curves)
            keys = list(curve_of)
            grid = np.stack([axis(int(blocks[curve_of[k]][0]), float(np.sqrt(bw["H"][curve_of[k]][0, 0])), g) for k in keys])
            res = launch(torch.from_numpy(grid).to(device), [curve_of[k] for k in keys], [np.array([r]) for r in range(len(keys))], True)
            dens = res["density"].cpu().numpy()
            out["curves"] = {v: [None] * v.dim for v in variables}
            for r, (v, c) in enumerate(keys):
                out["curves"][v][c] = dict(x=grid[r].astype(np.float64), density=dens[r].copy(),
                                           h=float(np.sqrt(bw["H"][curve_of[(v, c)]][0, 0])))
        if map_vars:
            gx, gy = int(maps[0]), int(maps[1])
            grid, axes = np.zeros((2 * len(map_vars), gx * gy), dtype=np.float32), {}
            for k, v in enumerate(map_vars):
                H = bw["H"][map_of[v]]
                ax = axis(pts.pcol[v], float(np.sqrt(H[0, 0])), gx)
                ay = axis(pts.pcol[v] + 1, float(np.sqrt(H[1, 1])), gy)
                axes[v] = (ax, ay)
                grid[2 * k], grid[2 * k + 1] = np.tile(ax, gy), np.repeat(ay, gx)
            res = launch(torch.from_numpy(grid).to(device), [map_of[v] for v in map_vars],
                         [np.array([2 * k, 2 * k + 1]) for k in range(len(map_vars))], True)
            dens = res["density"].cpu().numpy()
            out["maps"] = {v: dict(x=axes[v][0].astype(np.float64), y=axes[v][1].astype(np.float64), density=dens[k].reshape(gy, gx).copy(),
                                   H=bw["H"][map_of[v]].copy()) for k, v in enumerate(map_vars)}
        if at_keys:
            q = max(p.shape[0] for p in at_pts)                            # a launch has one m: shorter sets repeat their first point
            host = np.concatenate([np.vstack([p, np.repeat(p[:1], q - p.shape[0], axis=0)]).T for p in at_pts]).astype(np.float32)
            qcols, r = [], 0
            for p in at_pts:
                qcols.append(np.arange(r, r + p.shape[1]))
                r += p.shape[1]
            res = launch(torch.from_numpy(np.ascontiguousarray(host)).to(device), [index[blk] for blk in at_keys], qcols)
            ld = res["log_density"].cpu().numpy()
            out["log_density"] = {(blk if len(blk) == 2 else blk[0]): ld[k, :p.shape[0]].copy()
                                  for k, (blk, p) in enumerate(zip(at_keys, at_pts))}
        if graded:
            which = [index[(v,)] for v in graded]
            host = np.concatenate([np.asarray(truth[v], dtype=np.float32) for v in graded]).reshape(-1, 1)
            qcols, r = [], 0
            for v in graded:
                qcols.append(np.arange(r, r + v.dim))
                r += v.dim
            at_truth = launch(torch.from_numpy(host).to(device), which, qcols)["log_density"][:, 0]
            own = launch(St, which, [blocks[b] for b in which])["log_density"]
            level = torch.stack([ST.hpd_level(own[k], at_truth[k], w_dev) for k in range(len(graded))]).cpu().numpy()
            nl = (-at_truth).cpu().numpy()
            out["nlpd"] = {v: float(nl[k]) for k, v in enumerate(graded)}
            out["hpd_level"] = {v: float(level[k]) for k, v in enumerate(graded)}
            out["mean_nlpd"] = float(np.mean(nl))
            out["coverage"] = {lev: float(np.mean(level <= lev)) for lev in (0.5, 0.9, 0.95)}
        return out

    # ---- how far every sampled trajectory lies from the ground truth: aligned ATE and RPE ---------------------------------------
    def posterior_trajectory_error(self, truth, samples=None, n: int = None, poses=None, landmarks=None, align: str = "rigid",
                                   reflect: bool = False, weights=None, strides=(1,), quantiles=(0.05, 0.5, 0.95),
                                   threshold=None) -> dict:
        """The trajectory error of EVERY posterior sample against ground truth, computed on the device from the sample matrix
        the tree walk left there (nfisam_sample_trajectory_error / nfisam_sample_trajectory_rpe: a sample per lane, float32
        points, float64 arithmetic).  Each row of that matrix is one complete trajectory: it is aligned to the truth on its
        own (the planar Kabsch-Umeyama fit in closed form) and graded, so the result is the DISTRIBUTION of the absolute
        trajectory error over the hypotheses the posterior holds -- where the reference's Plaza scripts grade the posterior mean
        alone (example/slam/plaza_dataset/plaza_traj_performance_plot.py:112-114,196-198,282-293 with
        src/utils/Functions.py:53-71), a point that on a multi-modal posterior is no hypothesis at all.

        truth: variable -> [dim] ground truth.  samples, n: as in `posterior_summary` (None draws `n` points through the
        walk; otherwise what `posterior_log_pdf` accepts); the matrix stays on the device.  poses: the time-ordered
        trajectory (default: the variables of `physical_vars`, in their order, that have a circular third coordinate and
        appear in `truth`; nothing is selected by name).  landmarks: graded through the poses' transform, outside the
        alignment (default: the 2-column variables in `truth`).  align: "none", "rigid" or "similarity" (the least-squares
        scale); reflect: also try the mirrored fit.  weights: None, an [n] array or "importance" as in `posterior_summary`;
        they enter the aggregates (per_pose_rmse, summary, mean_trajectory) alone.  strides: the pose distances of the
        relative pose error (an empty list: none).  quantiles, threshold: of `summary`.
        -> dict: ate, heading_rms, landmark_rmse [n] (NaN without headings / landmarks), theta, scale [n], t [n, 2], reflected
        [n] bool, worst_pose (dict(index [n]: the position in `poses` of the pose farthest from its truth, value [n])),
        per_pose_rmse (variable -> sqrt(sum_i w_i |r_i|^2 / sum_i w_i), poses and landmarks: which stretch of the path is
        off), rpe ({stride: dict(trans [n], rot [n], pairs)}), summary (utils.Statistics.trajectory_error_summary of ate),
        mean_trajectory (dict(ate, landmark_rmse, R, c, t): the posterior MEAN -- nfisam_sample_moments' means -- aligned by
        utils.Functions.kabsch_umeyama on the host and graded: the reference script's number; under "rigid" its scale is set
        to 1, under "none" it is `posterior_summary`'s translation_rmse over the poses), poses, landmarks, n, ess.
        Raises RuntimeError when there is nothing to grade yet; ValueError when `truth` holds none of the poses, for a stride
        outside [1, poses), an unknown mode, bad weights, quantiles or truths -- before anything is launched."""
        from utils import Functions as FN
        from utils import Statistics as ST
        what = "posterior_trajectory_error"
        if align not in _nh.TRAJ_MODES:
            raise ValueError("%s: align is one of 'none', 'rigid', 'similarity', got %r" % (what, align))
        if not hasattr(truth, "__contains__") or not hasattr(truth, "__getitem__"):
            raise ValueError("%s: truth maps variables to their ground truth" % what)
        pts, importance, _, _ = self._summary_front(what, samples, n, None, None, weights)
        known = pts.pcol
        given = poses is not None
        if poses is None:
            poses = [v for v in self.physical_vars if v.dim == 3 and v.circular_dim_list[2] and v in truth and v in known]
        poses = list(poses)
        if landmarks is None:
            landmarks = [v for v in self.physical_vars if v.dim == 2 and v in truth and v in known and v not in poses]
        landmarks = list(landmarks)
        if not poses or (given and not any(v in truth for v in poses)):
            raise ValueError("%s: truth holds none of the poses" % what)
        for v in poses + landmarks:
            self._need_known(what, v, known)
            if v not in truth:
                raise ValueError("%s: truth lacks variable %s" % (what, v.name))
            if v.dim < 2 or np.ndim(truth[v]) != 1 or len(truth[v]) != v.dim or not np.all(np.isfinite(np.asarray(truth[v], dtype=np.float64))):
                raise ValueError("%s: truth of %s must be [%d] finite values with an xy part, got shape %s"
                                 % (what, v.name, v.dim, np.shape(truth[v])))
        if len(set(poses)) != len(poses):
            raise ValueError("%s: a pose is listed twice" % what)
        headed = [v.dim >= 3 and bool(v.circular_dim_list[2]) for v in poses]
        with _named(what):
            strides = ST.check_strides(strides, len(poses)) if len(tuple(strides)) else ()
        if strides and not all(headed):
            raise ValueError("%s: the relative pose error needs a heading on every pose; pass strides=()" % what)
        probs = np.asarray(quantiles, dtype=np.float64).reshape(-1)
        if not np.all((probs >= 0.0) & (probs <= 1.0)):
            raise ValueError("%s: quantiles is a list of probabilities in [0, 1]" % what)
        if threshold is not None and not float(threshold) > 0.0:
            raise ValueError("%s: threshold is a positive distance" % what)
        w_host = self._summary_weights(what, weights, importance, pts.rows)

        every = poses + landmarks
        P = len(poses)
        truth64 = [np.asarray(truth[v], dtype=np.float64) for v in every]
        entries = _nh.pack_traj_entries([known[v] for v in every], [known[v] + 1 for v in every],
                                        [known[v] + 2 if k < P and headed[k] else -1 for k, v in enumerate(every)],
                                        np.array([a[:2] for a in truth64]), [a[2] if a.size > 2 else 0.0 for a in truth64],
                                        landmark=np.arange(len(every)) >= P)
        _nh.check_traj_entries(entries, pts.total_dim, align)
        pairs = _nh.pack_traj_pairs(np.arange(P), strides) if strides else None
        if pairs is not None:
            _nh.check_traj_pairs(pairs, entries, len(strides))

        w_dev, ess = self._weights(what, pts, importance, w_host)
        res = ST.trajectory_error_t(pts.St, entries, align, reflect, w_dev, checked=True)
        rpe = ST._rpe_result(_nh.sample_trajectory_rpe_t(pts.St, entries, pairs, len(strides), checked=True), strides) if strides else {}
        # the posterior mean, graded the reference's way: the device's means, then the SVD fit on the host
        cols = np.array([known[v] + c for v in every for c in range(2)], dtype=np.int32)
        blocks = _nh.pack_moment_blocks(np.ones(cols.size, dtype=np.int64))
        mean_d, _, _ = _nh.sample_moments_t(pts.St, blocks, cols, None, w_dev)
        est = mean_d.cpu().numpy().reshape(-1, 2)
        ref = np.array([a[:2] for a in truth64])
        R, c, t = np.eye(2), 1.0, np.zeros(2)
        if align != "none":
            R, c, t = FN.kabsch_umeyama(ref[:P], est[:P], reflect=reflect)
            if align == "rigid":
                c, t = 1.0, ref[:P].mean(axis=0) - R @ est[:P].mean(axis=0)
        r2 = np.sum((ref - (c * est @ R.T + t)) ** 2, axis=1)
        w_np = None if w_dev is None else (w_dev.cpu().numpy() if torch.is_tensor(w_dev) else np.asarray(w_dev))
        out = dict(res)
        per_entry = out.pop("per_entry_rmse")
        out.pop("weight_sum")
        index, value = out.pop("worst_pose")
        out.update(worst_pose=dict(index=index, value=value), per_pose_rmse={v: float(per_entry[k]) for k, v in enumerate(every)},
                   rpe=rpe, summary=ST.trajectory_error_summary(res["ate"], w_np, probs, threshold),
                   mean_trajectory=dict(ate=float(np.sqrt(r2[:P].mean())),
                                        landmark_rmse=float(np.sqrt(r2[P:].mean())) if len(every) > P else float("nan"),
                                        R=R, c=float(c), t=t),
                   poses=poses, landmarks=landmarks, n=pts.rows, ess=ess)
        return out
