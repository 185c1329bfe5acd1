#!/usr/bin/env python3
"""Generate tests/golden/g14_karate_asym_train.npz by running the REAL reference's training loop
(IterativeEmbedder.update_similarity_measure, clane/embedder.py:249-289).

TEST INFRASTRUCTURE, like tools/make_bilinear_golden.py: runs only where the reference is mounted read-only at
/root/reference; only the resulting arrays are committed.  The reference's IterativeEmbedder cannot be constructed
(its __init__ fails), so the object is made with object.__new__ and given the attributes the method reads.  Its random
streams (DataLoader shuffle, Python `random`, CPU bernoulli) cannot be replayed from seeds and differ by dtype, so
`clane.embedder.DataLoader` and `torch.Tensor.bernoulli` are wrapped: an fp32 run RECORDS every batch and every Bernoulli
outcome, an fp64 run REPLAYS them.  Stored: X, the initial W, per step src / dst / linked / trial, the fp64 run's W
before every step, its per-step dW (the parameters' .grad before optimizer.step; zero for a step the
reference skips because no pair took part in the loss), its epoch losses and final W, and --
teacher-forced from each recorded fp64 W -- the reference's own fp32 single-step dW, with
grad_err_ref_f32 = max over steps of max|dW_f32 - dW_f64|.

Usage: python tools/make_train_golden.py
"""
from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "g14_karate_asym_train.npz"
D, X_SEED, PHI_SEED, LR, EPOCHS, BATCH = 16, 13, 7, 1e-2, 3, 4


def main() -> None:
    import random
    import torch
    np.Inf = np.inf  # noqa: NPY201 -- alias the reference needs (embedder.py:1)
    sys.path.insert(0, str(REF))
    import clane.embedder as E
    import clane.graph as G
    import clane.similarity as S

    karate = np.load(OUT.parent / "g2_karate_csr.npz", allow_pickle=True)
    root = Path(tempfile.mkdtemp(prefix="clane_train_gold_"))
    (root / "V").write_text("\n".join(str(v) for v in karate["vertex_ids"]) + "\n")
    (root / "E").write_text("\n".join(f"{s}\t{d}" for s, d in zip(karate["edge_src"], karate["edge_dst"])) + "\n")
    X = torch.normal(0, 1, [len(karate["vertex_ids"]), D], generator=torch.Generator().manual_seed(X_SEED))
    np.save(root / "C.npy", X.numpy())
    torch.manual_seed(PHI_SEED)
    sim0 = S.AsymmertricSimilarity(D)
    W0 = torch.cat([sim0.Phi_src.weight.detach(), sim0.Phi_dst.weight.detach()], 0).clone()

    record = {"batches": [], "trials": []}
    state = {"mode": "record", "b": 0, "t": 0}
    RealLoader, real_bernoulli, RealAdam = E.DataLoader, torch.Tensor.bernoulli, E.Adam

    class Loader:
        def __init__(self, *a, **k):
            k["pin_memory"] = False
            self.inner = RealLoader(*a, **k)

        def __iter__(self):
            if state["mode"] == "record":
                for batch in self.inner:
                    record["batches"].append(tuple(t.clone() for t in batch))
                    yield batch
            else:
                for _ in range(len(self.inner)):
                    batch = record["batches"][state["b"]]
                    state["b"] += 1
                    yield tuple(t.clone() for t in batch)

    def bernoulli(self, *a, **k):
        if state["mode"] == "record":
            out = real_bernoulli(self, *a, **k)
            record["trials"].append(out.detach().bool().clone())
            return out
        out = record["trials"][state["t"]].to(self.dtype)
        state["t"] += 1
        return out

    trace = {"W_before": [], "dW": []}

    class TracingAdam(RealAdam):
        def zero_grad(self, *a, **k):            # called at the top of EVERY step, also one that `continue`s
            ps = [p for g in self.param_groups for p in g["params"]]
            trace["W_before"].append(torch.cat([p.detach().clone() for p in ps], 0))
            trace["dW"].append(torch.zeros_like(trace["W_before"][-1]))      # stays zero when the step is skipped
            return super().zero_grad(*a, **k)

        def step(self, *a, **k):
            ps = [p for g in self.param_groups for p in g["params"]]
            trace["dW"][-1] = torch.cat([p.grad.detach().clone() for p in ps], 0)
            return super().step(*a, **k)

    def run(dtype, adam):
        g = G.Graph(root, embedding_dim=D)
        g.X = g.X.to(dtype)
        for v, x in zip(g.V, g.X):
            v.x = v.z = x
        sim = S.AsymmertricSimilarity(D).to(dtype)
        with torch.no_grad():
            sim.Phi_src.weight.copy_(W0[:D])
            sim.Phi_dst.weight.copy_(W0[D:])
        emb = object.__new__(E.IterativeEmbedder)
        emb.graph, emb.similarity_measure, emb.batch_size, emb.lr = g, sim, BATCH, LR
        emb.device, emb.epoch, emb.num_workers = torch.device("cpu"), EPOCHS, 0
        E.DataLoader, E.Adam, torch.Tensor.bernoulli = Loader, adam, bernoulli
        try:
            losses = emb.update_similarity_measure()
        finally:
            E.DataLoader, E.Adam, torch.Tensor.bernoulli = RealLoader, RealAdam, real_bernoulli
        W = torch.cat([sim.Phi_src.weight.detach(), sim.Phi_dst.weight.detach()], 0)
        return [float(l) for l in losses], W

    random.seed(5)
    torch.manual_seed(11)
    state["mode"] = "record"
    losses32, W32 = run(torch.float32, RealAdam)
    state.update(mode="replay", b=0, t=0)
    losses64, W64 = run(torch.float64, TracingAdam)
    n_steps = len(record["batches"])
    assert state["b"] == n_steps and state["t"] == n_steps
    assert len(trace["dW"]) == n_steps, (len(trace["dW"]), n_steps)

    # the reference's own fp32 single step, teacher-forced from each recorded fp64 W
    dW32 = []
    for i, (src, dst, linked) in enumerate(record["batches"]):
        sim = S.AsymmertricSimilarity(D)
        with torch.no_grad():
            sim.Phi_src.weight.copy_(trace["W_before"][i][:D].float())
            sim.Phi_dst.weight.copy_(trace["W_before"][i][D:].float())
        prob = sim(X[src], X[dst]).sigmoid()
        loss = prob.where(linked, 1 - prob).add(1e-10).log().neg()
        mask = linked.logical_xor(record["trials"][i])
        if not mask.any():                       # the step the reference skips (embedder.py:280-281): no gradient
            dW32.append(torch.zeros(2 * D, D))
            continue
        loss.masked_select(mask).mean().backward()
        dW32.append(torch.cat([sim.Phi_src.weight.grad, sim.Phi_dst.weight.grad], 0))
    dW32, dW64 = torch.stack(dW32), torch.stack(trace["dW"])
    err = float((dW32.double() - dW64).abs().max())
    np.savez_compressed(
        OUT,
        X=X.numpy(), W0=W0.numpy(),
        src=torch.stack([b[0] for b in record["batches"]]).numpy().astype(np.int64),
        dst=torch.stack([b[1] for b in record["batches"]]).numpy().astype(np.int64),
        linked=torch.stack([b[2] for b in record["batches"]]).numpy().astype(np.uint8),
        trial=torch.stack(record["trials"]).numpy().astype(np.uint8),
        W_before=torch.stack(trace["W_before"]).numpy(), dW_f64=dW64.numpy(), dW_ref_f32=dW32.numpy(),
        losses_f64=np.array(losses64), losses_f32=np.array(losses32), W_final_f64=W64.numpy(), W_final_f32=W32.numpy(),
        grad_err_ref_f32=np.float64(err), lr=np.float64(LR), epochs=np.int64(EPOCHS), batch_size=np.int64(BATCH),
    )
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): {n_steps} steps, losses f64 {losses64}, f32 {losses32}, "
          f"max|W32 - W64| = {float((W32.double() - W64).abs().max()):.3e}, grad_err_ref_f32 = {err:.3e}")


if __name__ == "__main__":
    main()
