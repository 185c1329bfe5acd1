#!/usr/bin/env python3
"""SHA-256 of every output buffer of the dense (MFMA) kernels on fixed non-integer float inputs, as one JSON object.

The integer-data tests of the suite cannot see a changed accumulation order (integer sums are order-free) and the
fp64-bound tests allow one.  Inside ONE build tests/test_gpu_dense_bits.py sees it: every dense kernel must form a dot
with the bits project_rows forms, so an order that differs between two kernels, two tiles or two places of a list fails
there.  An order that changes in every kernel alike passes it, and that is what this tool is for: run it on two builds
of the library and compare the files -- any differing digest is a changed bit.  It calls only the clane_amd._hip
wrappers, so the same file runs against an older checkout.

Usage: python tools/mfma_digest.py [--out FILE]
"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from clane_amd import _hip  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
TABLE = 300


def rnd(seed, shape, dtype, dev, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(dtype).to(dev)


def rint(seed, lo, hi, shape, dtype, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int64).to(dtype).to(dev)


def indices(seed, n, dev, table=TABLE):
    """n table rows, every 37th outside the table (-1 or past its end)."""
    idx = rint(seed, 0, table, (n,), torch.int64, "cpu")
    idx[5::37] = -1
    idx[11::37] = table + 5
    return idx.to(torch.int32).to(dev)


def sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _hip.require_gpu("cuda:0")
    k = _hip.kernels()
    out = {}

    for tag, T in DTYPES.items():
        acc = _hip.acc_dtype(T)

        # ---- projection and the pair step
        for d in (5, 16, 130):
            Z = rnd(1, (TABLE, d), T, dev)
            W = rnd(2, (2 * d, d), acc, dev, 0.3)
            Y = torch.zeros(TABLE, 2 * d, dtype=acc, device=dev)
            k.project_rows(Z, d, W, Y)
            out[f"project_rows/{tag}/d{d}/Y"] = sha(Y)

            B = 300
            src, dst = indices(3, B, dev), indices(4, B, dev)
            PA, PB = torch.zeros(B * d, dtype=acc, device=dev), torch.zeros(B * d, dtype=acc, device=dev)
            k.pair_project(Z, d, src, dst, W, PA, PB)
            out[f"pair_project/{tag}/d{d}/A"] = sha(PA)
            out[f"pair_project/{tag}/d{d}/B"] = sha(PB)

            B = 2100                                      # more than one chunk of pairs
            src, dst = indices(5, B, dev), indices(6, B, dev)
            PA, PB, g = rnd(7, (B * d,), acc, dev), rnd(8, (B * d,), acc, dev), rnd(9, (B,), acc, dev, 0.5)
            stats = torch.tensor([1.0, 97.0], dtype=torch.float64, device=dev)
            ws = torch.zeros(k.pair_grad_ws_len(B, d), dtype=acc, device=dev)
            dW = torch.zeros(2 * d * d, dtype=acc, device=dev)
            k.pair_grad(Z, d, src, dst, PA, PB, g, stats, ws, dW)
            out[f"pair_grad/{tag}/d{d}/dW"] = sha(dW)

        # ---- the probes
        for n in (300, 2100):
            for d in (5, 130):
                for C, F in ((7, 19), (33, 3)):
                    Z = rnd(11, (TABLE, d), T, dev)
                    rows = indices(12, n, dev)
                    split = rint(13, 0, 2, (n, F), torch.uint8, dev)
                    case = f"{tag}/n{n}/d{d}/C{C}F{F}"

                    K = F * _hip.probe_padded_classes(C)
                    W, bias = rnd(14, (K, d), acc, dev, 0.3), rnd(15, (K,), acc, dev, 0.3)
                    y = rint(16, 0, C, (n,), torch.int32, dev)
                    loss_ws = torch.zeros(k.probe_loss_ws_len(n, F), dtype=torch.float64, device=dev)
                    loss = torch.zeros(F, dtype=torch.float64, device=dev)
                    G = torch.zeros(n * K, dtype=acc, device=dev)
                    pred = torch.zeros(n, F, dtype=torch.int32, device=dev)
                    k.probe_forward(Z, d, rows, y, split, W, bias, F, C, loss_ws, loss, G=G, pred=pred)
                    for name, t in (("G", G), ("loss", loss), ("pred", pred)):
                        out[f"probe_forward/{case}/{name}"] = sha(t)

                    Gin = rnd(17, (n * K,), acc, dev, 0.5)
                    ws = torch.zeros(k.probe_grad_ws_len(n, K, d), dtype=acc, device=dev)
                    dW, db = torch.zeros(K * d, dtype=acc, device=dev), torch.zeros(K, dtype=acc, device=dev)
                    k.probe_grad(Z, d, rows, Gin, ws, dW, db)
                    out[f"probe_grad/{case}/dW"] = sha(dW)
                    out[f"probe_grad/{case}/db"] = sha(db)

                    K = F * _hip.ovr_padded_classes(C)
                    W, bias = rnd(18, (K, d), acc, dev, 0.3), rnd(19, (K,), acc, dev, 0.3)
                    bits = rint(20, 0, 4, (n, C), torch.int64, "cpu") == 0          # a quarter of the classes per row
                    ymask = (bits.long() << torch.arange(C)).sum(1).to(dev)
                    x = rint(21, 0, 8, (K,), torch.int64, "cpu")                    # an eighth of the columns -1, an eighth +1
                    col_state = ((x == 1).long() - (x == 0).long()).to(torch.int8).to(dev)
                    max_labels = int(bits.sum(1).max())
                    for top_k in (True, False):
                        loss_ws.zero_()
                        G = torch.zeros(n * K, dtype=acc, device=dev)
                        pred = torch.zeros(n, F, dtype=torch.int64, device=dev)
                        k.probe_forward_ovr(Z, d, rows, ymask, split, W, bias, col_state, F, C, max_labels, loss_ws, loss,
                                            G=G, pred=pred, top_k=top_k)
                        mode = "topk" if top_k else "threshold"
                        for name, t in (("G", G), ("loss", loss), ("pred", pred)):
                            out[f"probe_forward_ovr/{case}/{mode}/{name}"] = sha(t)

        # ---- ranking and evaluation
        for d in (5, 130):
            S, N = rnd(31, (TABLE, d), T, dev), rnd(32, (TABLE, d), T, dev)
            sq = (N.cpu().double() ** 2).sum(1).to(acc).to(dev)
            sums2 = torch.tensor([37.25, 1911.5], dtype=torch.float64, device=dev)
            label = rint(33, 0, 10 ** 6, (TABLE,), torch.int64, "cpu")
            label = (torch.arange(TABLE) * 7 + label % 7).to(torch.int32)          # unique
            label[3::41] = -1
            label = label.to(dev)
            deg = rint(34, 0, 9, (TABLE,), torch.int64, "cpu")
            rowptr = torch.zeros(TABLE + 1, dtype=torch.int64)
            rowptr[1:] = deg.cumsum(0)
            g = torch.Generator().manual_seed(35)
            colidx = torch.cat([torch.randperm(TABLE, generator=g)[:int(m)].sort().values for m in deg]).to(torch.int32)
            rowptr, colidx = rowptr.to(dev), colidx.to(dev)
            Q, kk = 70, 10
            q_rows, t_rows = indices(36, Q, dev), indices(37, Q, dev)
            for mname, mode in _hip.SCORE_MODES.items():
                s2 = sums2 if mode == _hip.SCORE_REFERENCE else None
                sqm = sq if mode == _hip.SCORE_PER_EDGE else None
                for n_slabs in (1, 3):
                    case = f"{tag}/d{d}/{mname}/slabs{n_slabs}"
                    cs = torch.zeros(Q * n_slabs * kk, dtype=acc, device=dev)
                    ci = torch.zeros(Q * n_slabs * kk, dtype=torch.int32, device=dev)
                    k.rank_scores(S, N, TABLE, d, q_rows, mode, s2, sqm, label, rowptr, colidx, True, kk, n_slabs, cs, ci)
                    os_ = torch.zeros(Q * kk, dtype=acc, device=dev)
                    oi = torch.zeros(Q * kk, dtype=torch.int32, device=dev)
                    k.rank_merge(cs, ci, n_slabs, kk, os_, oi)
                    for name, t in (("cand_score", cs), ("cand_id", ci), ("score", os_), ("id", oi)):
                        out[f"rank_scores/{case}/{name}"] = sha(t)
                    ts = torch.zeros(Q, dtype=acc, device=dev)
                    counts = torch.zeros(Q * n_slabs * 4, dtype=torch.int32, device=dev)
                    k.rank_count(S, N, TABLE, d, q_rows, t_rows, mode, s2, sqm, label, rowptr, colidx, True, n_slabs, ts,
                                 counts)
                    out[f"rank_count/{case}/target_score"] = sha(ts)
                    out[f"rank_count/{case}/counts"] = sha(counts)

        # ---- k-means assignment
        for d in (5, 130):
            for K in (7, 140):
                n, R = 300, 2
                Z = rnd(41, (TABLE, d), T, dev)
                rows = indices(42, n, dev)
                centres = rnd(43, (R, K, d), acc, dev)
                csq = (centres.cpu().double() ** 2).sum(2).to(acc).to(dev)
                assign = torch.zeros(n, R, dtype=torch.int32, device=dev)
                best = torch.zeros(n, R, dtype=acc, device=dev)
                k.kmeans_assign(Z, d, rows, centres, csq, assign, best)
                out[f"kmeans_assign/{tag}/d{d}/K{K}/assign"] = sha(assign)
                out[f"kmeans_assign/{tag}/d{d}/K{K}/best"] = sha(best)

    torch.cuda.synchronize()
    text = json.dumps(out, indent=0, sort_keys=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)
    print(f"{len(out)} digests", file=sys.stderr)


if __name__ == "__main__":
    main()
