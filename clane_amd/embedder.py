"""Embedder -- the reference's ``clane/embedder.py:12-108`` control flow over the GPU engine.

The constructor signature, ``iterate()`` / ``propagate()``, ``Tolerence``, ``tolerences``,
``history`` and ``minimum_amount_updated_Z`` are the reference's (including the spelling
``tolerence``).  What changed is where the work happens: ``build_P`` and every sweep
``Z <- X + gamma * P Z`` with its L1 delta run as HIP kernels on the ``SweepEngine``; the host
reads back one scalar per sweep to drive exactly the reference's stopping rule.
"""
from __future__ import annotations

import collections
import math
import os
import time
import queue
import threading
from pathlib import Path
from typing import Callable, Optional

import torch

from .graph import Graph
from .similarity import AsymmertricSimilarity, CosineSimilarity, Similarity


class Embedder(object):
    LAGGED_BELOW_S = 1e-3             # one GPU: the host check lags one sweep when a sweep is ESTIMATED below this
    # Several ranks decide by the engine's ESTIMATE of a sweep (gather-model bytes at the HBM peak), which measured
    # sweeps undercut by cache hits (config 3: 0.65-0.85 of it at N = 1..8): 2 ms of estimate is ~1.3-1.7 ms of sweep,
    # where the host round trip plus the scalar all-reduce (~50 us) is 3 % or more.
    LAGGED_BELOW_ESTIMATE_S = 2e-3

    def __init__(
        self,
        graph:              Graph,
        similarity_measure: Similarity,
        device,
        gamma:              float = 0.76,
        tolerence:          int = 10,
        batch_size:         int = 4,
        lr:                 float = 1e-4,
        num_workers:        int = 0,
        save_history:       bool = False,
        verbose:            bool = True,
        max_sweeps:         Optional[int] = None,
        history_sink:       Optional[Callable[[int, int, torch.Tensor], None]] = None,
        history_parts_dir=None,
        skip_idle_sweeps:   bool = True,
        lagged_check:       Optional[bool] = None,
    ) -> None:
        self.graph = graph
        self.similarity_measure = similarity_measure
        self.device = device
        self.gamma = gamma
        self.tolerences = {
            "global": self.Tolerence(tolerence),
            "propagation": self.Tolerence(tolerence),
            "similarity_model": self.Tolerence(tolerence),
        }
        self.batch_size = batch_size
        self.lr = lr
        self.num_workers = num_workers
        self.save_history = save_history
        if save_history:
            self.history = {"Z": [], "loss_P": []}
        self.minimum_amount_updated_Z = math.inf
        # extensions (default = reference behaviour)
        self.verbose = verbose
        self.max_sweeps = max_sweeps          # safety cap per propagate(); None = reference (uncapped)
        self.sweep_counts = []
        self.outer_deltas = []
        # A sweep whose delta is exactly 0 reproduced its input bit for bit; with P frozen every further sweep of
        # the propagate is the same computation on the same data (the kernels are deterministic), so its delta is
        # 0 too.  Such sweeps are accounted (tolerance countdown, printout, history) without being launched -- at
        # the fp32 fixed point the reference's rule still asks for `tolerence` sweeps in each of `tolerence` rounds.
        self.skip_idle_sweeps = skip_idle_sweeps
        # lagged_check: the next sweep is launched before the host has read this sweep's delta, so the
        # GPU never waits for the host.  The stopping rule is unchanged: when it says stop, the sweep launched ahead
        # is discarded (the ping-pong partner still holds the right embeddings) -- counts, deltas and embeddings are
        # bit-identical either way.  It costs one discarded sweep per propagate and saves the host round trip of
        # every sweep, so it pays when sweeps are short.  None (default): on when the engine's estimate of a sweep (the
        # same number on every rank and in every run) is below LAGGED_BELOW_S on one GPU, LAGGED_BELOW_ESTIMATE_S on
        # several; True / False: always / never.  Off with save_history.
        self.lagged_check = lagged_check
        self.sweeps_launched = 0
        self._round_was_idle = False
        # dtype the reference's per-sweep delta would have (the sum of |Z_new - Z_old| in Z's dtype): only its printout
        x_dtype = getattr(getattr(graph, "X", None), "dtype", torch.float32)
        self._delta_dtype = x_dtype if x_dtype in (torch.float32, torch.float64) else torch.float32
        # history_sink(outer, sweep, Z): with save_history, every sweep's embeddings are handed to it from a
        # writer thread, in order, instead of being kept in `history["Z"]` -- the copy to the host overlaps the
        # following sweeps (SweepEngine.stage_Z).  Call flush_history() (iterate() does) before relying on it.
        # history_parts_dir (several GPUs): a directory every rank of the box can write.  Each rank then stages only
        # the part of Z it holds (SweepEngine.stage_Z(pieces=True): no collective, N PCIe links in parallel), its
        # writer thread drops the part there, and rank 0's writer thread puts the parts together for the sink -- the
        # sweeps do not wait for any of it.  Without it a multi-GPU run gathers Z synchronously for every sweep.
        self._parts_dir = Path(history_parts_dir) if history_parts_dir is not None else None
        self._writer = _HistoryWriter(history_sink) if (save_history and history_sink is not None) else None

    class Tolerence:
        """Countdown of consecutive non-improving steps (reference embedder.py:45-54)."""

        def __init__(self, initial_value):
            self.initial_value = initial_value
            self.value = initial_value

        def reset(self):
            self.value = self.initial_value

        def endure(self):
            self.value -= 1

    # ------------------------------------------------------------------------------------
    def _engine(self):
        sim = self.similarity_measure
        if isinstance(sim, CosineSimilarity):
            return self.graph.engine(self.device, cosine_mode=sim.mode)
        # a plug-in similarity (and the bilinear AsymmertricSimilarity) needs whole rows: should this call be the one
        # that creates the engine of a multi-GPU run, it divides the rows (an engine that exists already keeps its division)
        return self.graph.engine(self.device, exchange=self.graph.PLUGIN_EXCHANGE)

    def _build_P(self, engine) -> None:
        if isinstance(self.similarity_measure, CosineSimilarity):
            engine.build_P()                              # fused K0+K1+K2
        elif isinstance(self.similarity_measure, AsymmertricSimilarity):
            self.graph._build_P_bilinear(engine, self.similarity_measure)   # projection + pair K1, P stays on the card
        else:
            self.graph.build_P(self.similarity_measure)   # plugin callable + HIP softmax

    # ---- training the similarity (reference embedder.py:249-289) --------------------------------------------------
    def _pair_sampler(self, engine):
        """The sampler of this embedder's own training calls: made once, so that successive calls draw new epochs."""
        if getattr(self, "_sampler", None) is None or self._sampler.eng is not engine:
            from .train import PairSampler
            gen = torch.Generator(device=engine.device)
            gen.manual_seed(int(getattr(self, "seed", 0)))
            self._sampler = PairSampler(engine, self.batch_size, gen, float(getattr(self, "positive_fraction", 0.0)))
        return self._sampler

    def update_similarity_measure(self, epochs: Optional[int] = None, sampler=None, replay=None):
        """Train the AsymmertricSimilarity on the current embeddings for ``epochs`` epochs (default: ``self.epoch``, else 1)
        with a fresh Adam (the reference builds a new optimizer per call, embedder.py:259) and return the per-epoch
        losses as the reference reports them: the sum of the step losses over the index of the epoch's last step
        (embedder.py:287; a one-step epoch divides by 1).  The steps run in HIP kernels on the engine; the host reads one
        scalar per epoch.  Afterwards the weights are copied back into ``Phi_src.weight`` / ``Phi_dst.weight``.

        ``sampler``: a ``train.PairSampler`` (default: one seeded with ``self.seed``, kept between calls).
        ``replay``: [(src, dst, linked, trial), ...] in VERTEX ids -- exactly these steps are run instead,
        ``len(replay) / epochs`` per epoch; ``trial`` holds the recorded Bernoulli outcomes (embedder.py:278)."""
        from .train import require_one_gpu, rows_of_vertices
        sim = self.similarity_measure
        if not isinstance(sim, AsymmertricSimilarity):
            raise TypeError(f"update_similarity_measure trains an AsymmertricSimilarity, not a {type(sim).__name__}")
        engine = self._engine()
        require_one_gpu(engine)
        if sim.Phi_src.in_features != engine.d_full:
            raise ValueError(f"AsymmertricSimilarity(n_dim={sim.Phi_src.in_features}) does not fit embeddings of "
                             f"dimension {engine.d_full}")
        epochs = int(getattr(self, "epoch", 1) if epochs is None else epochs)
        if epochs < 1:
            raise ValueError("update_similarity_measure: at least one epoch")
        W0 = sim.stacked_weight(engine.acc_dtype, engine.device)
        if replay is not None:
            if len(replay) == 0 or len(replay) % epochs:
                raise ValueError(f"replay: {len(replay)} steps do not divide into {epochs} epochs")
            dev, acc = engine.device, engine.acc_dtype
            steps = [(rows_of_vertices(engine, s), rows_of_vertices(engine, t),
                      torch.as_tensor(l).to(dev, torch.uint8).contiguous(),
                      # a recorded success is replayed with u = 0 (0 < p), a failure with u = 1 (1 < p never holds)
                      1.0 - torch.as_tensor(b).to(dev, acc).contiguous()) for s, t, l, b in replay]
            per_epoch = len(steps) // epochs
            trainer = engine.similarity_trainer(W0, self.lr, max(s[0].numel() for s in steps))
            batches = lambda e: steps[e * per_epoch:(e + 1) * per_epoch]     # noqa: E731
        else:
            sampler = sampler if sampler is not None else self._pair_sampler(engine)
            trainer = engine.similarity_trainer(W0, self.lr, sampler.batch_size)
            batches = lambda e: sampler.epoch()                              # noqa: E731
        losses = []
        for e in range(epochs):
            n_steps = 0
            for src, dst, linked, u in batches(e):
                trainer.step(src, dst, linked, u)
                n_steps += 1
            losses.append(trainer.epoch_loss() / max(n_steps - 1, 1))
        W = trainer.weights()
        d = engine.d_full
        with torch.no_grad():
            sim.Phi_src.weight.copy_(W[:d].to(sim.Phi_src.weight.device, sim.Phi_src.weight.dtype))
            sim.Phi_dst.weight.copy_(W[d:].to(sim.Phi_dst.weight.device, sim.Phi_dst.weight.dtype))
        self.last_trainer = trainer
        return losses

    def iterate(self):
        """Outer fixed point (reference embedder.py:56-69)."""
        engine = self._engine()
        replay = False
        while True:
            if not replay:
                engine.snapshot()
            self.propagate(_replay=replay)
            amount_updated_Z_current = 0.0 if replay else engine.distance_from_snapshot()
            self.outer_deltas.append(amount_updated_Z_current)

            if self.minimum_amount_updated_Z > amount_updated_Z_current:
                self.tolerences['global'].reset()
                self.minimum_amount_updated_Z = amount_updated_Z_current
            else:
                self.tolerences['global'].endure()

            if self.tolerences['global'].value == 0:  # embeddings are no more updated
                break
            # A round whose FIRST sweep already had delta 0 changed nothing at all; the built-in CosineSimilarity is
            # a deterministic function of Z, so the next round would rebuild the same P and repeat the same sweeps
            # bit for bit: it is accounted (counts, countdown, printout, history) without being launched.
            replay = (self.skip_idle_sweeps and isinstance(self.similarity_measure, CosineSimilarity)
                      and self._round_was_idle and amount_updated_Z_current == 0.0)
        self.flush_history()

    def flush_history(self) -> None:
        """Wait until the history sink has received everything handed to it so far."""
        if self._writer is not None:
            self._writer.flush()

    def _stage(self, engine, world: int):
        """This sweep's embeddings on their way to the host."""
        pieces = world > 1 and self._writer is not None and self._parts_dir is not None
        if pieces and self._writer.assembler is None:
            # a directory of this run's own (rank 0 names it, every rank learns the name: a collective, on this -- the
            # sweep's -- thread, where all ranks are in step): parts an interrupted run left behind cannot be mistaken
            run = engine.comm.all_gather_object(f"run-{os.getpid()}-{time.time_ns()}")[0]
            self._writer.assembler = _PartsAssembler(self._parts_dir / run, engine.comm.rank, world,
                                                     (engine.V, engine.d_full), engine.dtype)
            self._writer.assembler.check_shared(engine.comm)
        return engine.stage_Z(pieces=True) if pieces else engine.stage_Z()

    @torch.no_grad()
    def propagate(self, _replay: bool = False):
        """Jacobi sweeps with P frozen until `tolerence` consecutive sweeps bring no new
        minimum of the L1 delta (reference embedder.py:71-108).  `_replay` (iterate() only): the round is known
        to repeat an all-idle one -- nothing is launched, everything is accounted."""
        engine = self._engine()
        if not _replay:
            self._build_P(engine)
        minimum_amount_updated = math.inf
        self.tolerences['propagation'].reset()
        history_Z = []
        in_flight = collections.deque()         # StagedZ not yet resolved (save_history without a sink)
        outer = len(self.sweep_counts)
        n_sweeps = 0

        idle = _replay
        staged = None
        self._round_was_idle = False
        can_lag = not self.save_history
        ahead = bool(self.lagged_check) and can_lag
        world = engine.world
        if self.lagged_check is None and can_lag:
            # decided by the engine's estimate of a sweep, not by a stopwatch: several ranks must decide alike (the
            # estimate is the same number on every rank), and on one GPU the number of launches of a run is then the
            # same from run to run (round 2 switched by measured sweep times).  Lagging also hides the latency of the
            # per-sweep scalar all-reduce, hence the higher limit on several GPUs.
            limit = self.LAGGED_BELOW_ESTIMATE_S if world > 1 else self.LAGGED_BELOW_S
            ahead = engine.estimated_sweep_seconds() < limit
        ticket = None                               # the launched sweep whose delta has not been read yet
        if ahead and not idle:
            ticket = engine.sweep_launch(self.gamma)
            self.sweeps_launched += 1
        while True:
            if idle:
                amount_updated = 0.0
            elif ahead:
                following = engine.sweep_launch(self.gamma)         # runs while the host reads and decides
                amount_updated = engine.sweep_wait(ticket)
                ticket = following
            else:
                amount_updated = engine.sweep(self.gamma)
                self.sweeps_launched += 1
            n_sweeps += 1
            if self.save_history:
                if not idle or staged is None:      # an idle sweep leaves the embeddings as they are: same copy
                    staged = self._stage(engine, world)
                if self._writer is not None:
                    self._writer.submit(outer, n_sweeps - 1, staged)
                else:                           # reference behaviour: keep every Z; resolve copies as slots run out
                    in_flight.append((len(history_Z), staged))
                    history_Z.append(None)
                    while len(in_flight) >= engine.STAGE_SLOTS:
                        i, st = in_flight.popleft()
                        history_Z[i] = st.result()

            if minimum_amount_updated > amount_updated:
                self.tolerences['propagation'].reset()
                minimum_amount_updated = amount_updated
            else:
                self.tolerences['propagation'].endure()

            stop = self.tolerences['propagation'].value == 0 or bool(self.max_sweeps and n_sweeps >= self.max_sweeps)
            if self.skip_idle_sweeps and amount_updated == 0.0:
                idle = True
                if n_sweeps == 1:
                    self._round_was_idle = True
            if ahead and ticket is not None:
                if stop or idle:                    # the sweep launched ahead is not wanted
                    engine.discard_launch()
                    ticket = None
                else:
                    self.sweeps_launched += 1
            if self.verbose:        # the reference prints the 0-d tensor itself (embedder.py:104): "tensor(25.7074) 10"
                shown = torch.tensor(amount_updated, dtype=self._delta_dtype)
                print(shown, self.tolerences['propagation'].value)
            if self.tolerences['propagation'].value == 0 or (self.max_sweeps and n_sweeps >= self.max_sweeps):
                if self.save_history:
                    for i, st in in_flight:
                        history_Z[i] = st.result()
                    self.history['Z'].append(history_Z)
                self.sweep_counts.append(n_sweeps)
                return


class _PartsAssembler:
    """Several GPUs, one box: every rank's writer thread saves the part of Z it staged as a file in a directory
    they all see; rank 0's writer thread waits for the N parts of a sweep, puts them together (``place_piece``) and
    removes them.  No collective runs on a side thread, nothing runs on the sweep's stream."""
    # how long rank 0 waits for another rank's part of one sweep (a rank that FAILS says so at once, see `fail`; this
    # only bounds the wait for a rank that died without a word); CLANE_HISTORY_PATIENCE_S overrides
    PATIENCE_S = float(os.environ.get("CLANE_HISTORY_PATIENCE_S", "120"))

    def __init__(self, parts_dir: Path, rank: int, world: int, shape, dtype: torch.dtype):
        self.dir, self.rank, self.world, self.shape, self.dtype = Path(parts_dir), rank, world, tuple(shape), dtype
        self.dir.mkdir(parents=True, exist_ok=True)

    def check_shared(self, comm) -> None:
        """All ranks must see ONE directory (one box, one file system): rank 0 drops a token, everybody looks for it.
        Collective -- called once, on the sweep's thread, where the ranks are in step."""
        token = self.dir / "shared.token"
        if self.rank == 0:
            token.write_text("clane")
        comm.all_gather_object(self.rank)                   # rank 0 has written before anyone looks
        seen = comm.all_gather_object(token.exists())
        if self.rank == 0:
            token.unlink()
        if not all(seen):
            raise RuntimeError(f"--save_history on several GPUs hands the ranks' parts of Z over through {self.dir}, which "
                               f"ranks {[q for q, ok in enumerate(seen) if not ok]} do not see: the ranks must share a file "
                               f"system (one box)")

    def _path(self, outer: int, sweep: int, rank: int) -> Path:
        return self.dir / f"o{outer}_s{sweep}.r{rank}.pt"

    def fail(self, outer: int, sweep: int, exc: BaseException) -> None:
        """This rank cannot deliver its part: leave a marker rank 0 finds at once instead of waiting out its patience."""
        try:
            self._path(outer, sweep, self.rank).with_suffix(".err").write_text(f"{type(exc).__name__}: {exc}")
        except OSError:
            pass

    def collect(self, outer: int, sweep: int, staged):
        """Save this rank's part; rank 0: the whole [V, d] matrix of that sweep, the other ranks: None."""
        mine = self._path(outer, sweep, self.rank)
        tmp = mine.with_suffix(".tmp")
        try:
            torch.save(staged.piece(), tmp)
            tmp.rename(mine)                    # a part is either absent or complete
        except BaseException as exc:
            self.fail(outer, sweep, exc)
            raise
        if self.rank != 0:
            return None
        from .engine import place_piece
        Z = torch.empty(self.shape, dtype=self.dtype)
        deadline = time.monotonic() + self.PATIENCE_S
        for q in range(self.world):
            path = self._path(outer, sweep, q)
            while not path.exists():
                marker = path.with_suffix(".err")
                if marker.exists():
                    raise RuntimeError(f"history: rank {q} could not deliver its part of round {outer} sweep {sweep}: "
                                       f"{marker.read_text()}")
                if time.monotonic() > deadline:
                    raise TimeoutError(f"history: rank {q}'s part of round {outer} sweep {sweep} never arrived in "
                                       f"{self.dir} within {self.PATIENCE_S:.0f} s")
                time.sleep(0.002)
            place_piece(Z, torch.load(path))
            path.unlink()
        return Z


class _HistoryWriter:
    """One thread that resolves staged copies in order and hands them to the sink."""

    def __init__(self, sink):
        self.sink, self.q, self.error = sink, queue.Queue(), None
        self.assembler: Optional[_PartsAssembler] = None
        self.thread = threading.Thread(target=self._run, name="clane-history", daemon=True)
        self.thread.start()

    def _run(self):
        while True:
            outer, sweep, staged = self.q.get()
            try:
                # always resolve: frees the staging slot even after an error
                Z = staged.result() if getattr(staged, "_where", None) is None else self.assembler.collect(outer, sweep, staged)
                if self.error is None and Z is not None:
                    self.sink(outer, sweep, Z)
            except BaseException as exc:        # surfaced by flush()
                self.error = self.error or exc
            finally:
                self.q.task_done()

    def submit(self, outer, sweep, staged):
        if self.error is not None:
            self.flush()
        self.q.put((outer, sweep, staged))

    def flush(self):
        self.q.join()
        if self.error is not None:
            err, self.error = self.error, None
            raise RuntimeError("history sink failed") from err


class IterativeEmbedder(Embedder):
    """Placeholder for the reference's trainable-similarity embedder (embedder.py:158-289).

    Upstream it raises TypeError at construction (it calls ``Embedder.__init__`` without the
    required ``device``) and no passing test pins it, so it is out of scope here.
    """

    def __init__(self, *args, **kwargs) -> None:
        raise NotImplementedError(
            "IterativeEmbedder (trainable AsymmertricSimilarity) is not part of the MI355X hot path; the "
            "reference's own implementation fails at construction. Use CosineSimilarity with Embedder.")


class AlternatingEmbedder(Embedder):
    """Alternate "train the similarity" and "propagate with it" -- what the reference's ``IterativeEmbedder``
    (embedder.py:158-247) sets out to do, as a class of its own: upstream's fails in ``__init__`` and calls a method
    that does not exist, and ``IterativeEmbedder`` above stays the stub it was.  Hyper-parameter names are the
    reference's.  One round:

    1. ``update_similarity_measure(epoch)`` until ``tolerence_P`` consecutive calls bring no new minimum of the last
       epoch's loss (embedder.py:206-218);
    2. ``propagate()``: P from the new weights (``build_P_bilinear``) and sweeps until ``tolerence_Z`` consecutive
       sweeps bring no new minimum of the L1 delta (what ``update_embeddings`` evidently meant);
    3. the global rule of ``Embedder.iterate``: the distance of the embeddings from the round's start, ``tolerence``
       rounds without a new minimum end the run (``max_rounds`` caps it).

    Records ``train_losses`` (per round: the per-epoch losses of every training call), ``sweep_counts`` and
    ``outer_deltas``.  One GPU only."""

    def __init__(self, graph, similarity_measure, device, gamma: float = 0.76, tolerence: int = 10,
                 tolerence_Z: Optional[int] = None, tolerence_P: int = 1, epoch: int = 1, batch_size: int = 4,
                 lr: float = 1e-4, seed: int = 0, positive_fraction: float = 0.0, max_rounds: Optional[int] = None,
                 num_workers: int = 0, save_history: bool = False, verbose: bool = True,
                 max_sweeps: Optional[int] = None, **embedder_kwargs) -> None:
        if not isinstance(similarity_measure, AsymmertricSimilarity):
            raise TypeError(f"AlternatingEmbedder trains an AsymmertricSimilarity, not a "
                            f"{type(similarity_measure).__name__}")
        super().__init__(graph, similarity_measure, device, gamma=gamma, tolerence=tolerence, batch_size=batch_size,
                         lr=lr, num_workers=num_workers, save_history=save_history, verbose=verbose,
                         max_sweeps=max_sweeps, **embedder_kwargs)
        self.tolerence = tolerence
        self.tolerence_Z = tolerence if tolerence_Z is None else tolerence_Z
        self.tolerence_P = tolerence_P
        if min(self.tolerence, self.tolerence_Z, self.tolerence_P, epoch) < 1:
            raise ValueError("AlternatingEmbedder: tolerence, tolerence_Z, tolerence_P and epoch must be at least 1")
        self.tolerences["propagation"] = self.Tolerence(self.tolerence_Z)
        self.tolerences["similarity_model"] = self.Tolerence(self.tolerence_P)
        self.epoch, self.seed, self.positive_fraction, self.max_rounds = epoch, seed, positive_fraction, max_rounds
        self.train_losses = []

    def train_similarity(self):
        """Step 1 of a round; returns the per-epoch losses of every call it made."""
        tol = self.tolerences["similarity_model"]
        tol.reset()
        best, calls = math.inf, []
        while True:
            losses = self.update_similarity_measure(self.epoch)
            calls.append(losses)
            if losses[-1] >= best or math.isnan(losses[-1]):
                tol.endure()
            else:
                best = losses[-1]
                tol.reset()
            if self.verbose:
                print(f"similarity loss {losses[-1]:.6f}", tol.value)
            if tol.value == 0:
                return calls

    def iterate(self):
        engine = self._engine()
        from .train import require_one_gpu
        require_one_gpu(engine)
        rounds = 0
        while True:
            engine.snapshot()
            self.train_losses.append(self.train_similarity())
            self.propagate()
            amount = engine.distance_from_snapshot()
            self.outer_deltas.append(amount)
            if self.minimum_amount_updated_Z > amount:
                self.tolerences["global"].reset()
                self.minimum_amount_updated_Z = amount
            else:
                self.tolerences["global"].endure()
            rounds += 1
            if self.tolerences["global"].value == 0 or (self.max_rounds and rounds >= self.max_rounds):
                break
        self.flush_history()
