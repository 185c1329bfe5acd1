"""CLI -- ``python -m clane_amd [embedding] --data_root D --output_root O --config_file C``.

Mirrors the reference's ``clane/__main__.py`` (same flags, same YAML keys, same outputs:
``output_root/Z.npy`` and, with ``--save_history``, ``output_root/{outer}/Z_{sweep}.npy``).
The README form ``clane embedding ...`` (README.md:11) is accepted too: the reference's parser
rejects the ``embedding`` token, here it is an optional no-op.  The loop always
runs on the GPU; ``--gpu`` only selects where ``Embedder.device`` points, as upstream.
"""
from __future__ import annotations

import argparse
import os
import shutil
from pathlib import Path

import numpy as np
import torch
import yaml

from . import similarity
from .embedder import AlternatingEmbedder, Embedder, IterativeEmbedder
from .graph import Graph


def _distributed_setup():
    """Under `torchrun --nproc-per-node N` (WORLD_SIZE > 1): one process per GPU, RCCL process group.
    Returns (rank, world).  A plain `python -m clane_amd` run is (0, 1) and touches nothing.
    Rehearsal on a one-GPU box: CLANE_DIST_BACKEND=gloo CLANE_SHARE_GPU=1 (RCCL refuses two ranks on one device)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return 0, 1
    import torch.distributed as dist
    local_rank = 0 if os.environ.get("CLANE_SHARE_GPU") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.device_count() == 1:              # the launcher masked the devices per process
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if not dist.is_initialized():
        if os.environ.get("CLANE_DIST_BACKEND", "nccl") == "gloo":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    return dist.get_rank(), world


def embedding(args):
    predict_k = getattr(args, "predict_links", None)
    if predict_k is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:       # before any work, as --train_similarity
        raise NotImplementedError("--predict_links runs on one GPU only; several GPUs are out of scope")
    if predict_k is None and getattr(args, "link_sources", None) is not None:
        raise ValueError("--link_sources restricts --predict_links; give that flag too")
    if args.config_file.absolute().exists():
        with open(args.config_file.absolute(), 'r') as config_io:
            hparams = yaml.load(config_io, Loader=yaml.FullLoader)
    else:
        raise FileNotFoundError(f"Config file not found. {args.config_file.absolute()}")
    # optional section (extension): link_evaluation: {pairs: held_out.tsv, hits: [1, 3, 10], filter_existing: true}
    link_eval = hparams.get("link_evaluation") if isinstance(hparams, dict) else None
    if link_eval is not None:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:                    # before any work, as --predict_links
            raise NotImplementedError("link_evaluation runs on one GPU only; several GPUs are out of scope")
        if not isinstance(link_eval, dict) or "pairs" not in link_eval:
            raise ValueError("link_evaluation: the section needs 'pairs', the file of held-out src<TAB>dst lines")
    # optional section (extension): node_classification: {labels: Y, ratios: [..], runs: 10, seed: 0, l2: 1.0, baseline: true,
    # multilabel: true, predict: top_k | threshold}
    node_cls = hparams.get("node_classification") if isinstance(hparams, dict) else None
    if node_cls is not None:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:                    # before any work, as link_evaluation
            raise NotImplementedError("node_classification runs on one GPU only; several GPUs are out of scope")
        if not isinstance(node_cls, dict) or "labels" not in node_cls:
            raise ValueError("node_classification: the section needs 'labels', the file of id<TAB>class lines")
        if not isinstance(node_cls.get("multilabel", False), bool):
            raise ValueError(f"node_classification: multilabel must be true or false, got {node_cls['multilabel']!r}")
        if node_cls.get("predict", "top_k") not in ("top_k", "threshold"):
            raise ValueError(f"node_classification: predict must be top_k or threshold, got {node_cls['predict']!r}")
        if "predict" in node_cls and not node_cls.get("multilabel", False):
            raise ValueError("node_classification: predict belongs to multilabel: true")
    # optional section (extension): node_clustering: {labels: Y, clusters: 7, restarts: 10, seed: 0, max_iter: 300,
    # baseline: true, assignments: true}
    node_clu = hparams.get("node_clustering") if isinstance(hparams, dict) else None
    if node_clu is not None:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:                    # before any work, as node_classification
            raise NotImplementedError("node_clustering runs on one GPU only; several GPUs are out of scope")
        if not isinstance(node_clu, dict) or ("labels" not in node_clu and "clusters" not in node_clu):
            raise ValueError("node_clustering: the section needs 'labels', the file of id<TAB>class lines, or 'clusters', "
                             "the number of clusters")
        # scoring without labels: silhouette: true, silhouette_metric, silhouette_points; clusters may be a list (cluster.py)
        from . import cluster as cluster_mod
        node_clu_scoring = cluster_mod.check_section(node_clu)
    # optional section (extension): content_reduction: {dim: 128, center: true, whiten: false, load: pca.npz} -- the
    # content's principal components instead of the content (reduce.py); checked before the graph loads.  With
    # sparse: C.npz (and oversample / power_iterations / seed) the content is a CSR bag of words, read and validated here
    reduction = hparams.get("content_reduction") if isinstance(hparams, dict) else None
    reduction_file = sparse_content = None
    if reduction is not None:
        from . import reduce
        reduction = reduce.check_section(reduction, int(os.environ.get("WORLD_SIZE", "1")))
        reduction_file = reduce.resolve_load(reduction, Path(args.data_root))
        sparse_content = reduce.resolve_sparse(reduction, Path(args.data_root))
        if sparse_content is not None:
            from .graph import read_vertex_ids
            n_vertices = len(read_vertex_ids(Path(args.data_root)))
            if sparse_content.shape[0] != n_vertices:
                raise ValueError(f"content_reduction: sparse: the file holds {sparse_content.shape[0]} rows, V lists "
                                 f"{n_vertices} vertices")
    # optional section (extension): new_vertices: {root: arrivals, max_rounds: 64, weights: true} -- vertices that are not
    # in V, embedded against the finished graph (induct.py); everything about the files is checked before the graph loads
    new_vertices = hparams.get("new_vertices") if isinstance(hparams, dict) else None
    arrivals = None
    if new_vertices is not None:
        from . import induct
        from .graph import read_vertex_ids
        new_vertices = induct.check_section(new_vertices, int(os.environ.get("WORLD_SIZE", "1")))
        arrivals_root = Path(new_vertices["root"])
        if not arrivals_root.is_absolute():
            arrivals_root = Path(args.data_root) / arrivals_root
        arrivals = induct.read_arrivals(arrivals_root, read_vertex_ids(Path(args.data_root)), None)
    # optional section (extension): layout: {perplexity: 30, max_points: 20000, max_iter: 1000, seed: 0, labels: Y,
    # baseline: true, method: exact | neighbours, neighbours: K} -- the 2-D t-SNE picture of the embeddings the run ends
    # with (layout.py); checked before the graph loads
    layout_cfg = layout_labels = None
    if isinstance(hparams, dict) and "layout" in hparams:
        from . import layout as layout_mod
        layout_cfg = layout_mod.check_section(hparams["layout"], int(os.environ.get("WORLD_SIZE", "1")))
        layout_labels = layout_mod.resolve_labels(layout_cfg, Path(args.data_root))

    # optional section (extension): label_prediction: {labels: Y | load: label_model.npz, l2: 1.0 | [..], folds: 5, seed: 0,
    # top: 3, multilabel: false, scope: unlabelled | all} -- a kept classifier on the embeddings the run ends with and its
    # predictions for the other vertices (classify.py); checked before the graph loads
    label_pred = None
    if isinstance(hparams, dict) and "label_prediction" in hparams:
        from . import classify
        label_pred = classify.check_section(hparams["label_prediction"], Path(args.data_root),
                                            int(os.environ.get("WORLD_SIZE", "1")))

    # optional section (extension): soft_clustering: {clusters: 5 | [..], labels: Y, restarts: 10, seed: 0, max_iter: 100,
    # tol: 0.001, reg_covar: 1.0e-6, criterion: bic | aic, baseline: true, memberships: true, top: 3} -- a Gaussian
    # mixture on the embeddings the run ends with (mixture.py); checked before the graph loads
    soft_clu = None
    if isinstance(hparams, dict) and "soft_clustering" in hparams:
        from . import mixture
        soft_clu = mixture.check_section(hparams["soft_clustering"], Path(args.data_root),
                                         int(os.environ.get("WORLD_SIZE", "1")))

    rank, world = _distributed_setup()
    say = print if rank == 0 else (lambda *a, **k: None)      # every rank computes; rank 0 talks and writes
    say('[Embedding]', end='\n')

    device = torch.device('cuda') if args.gpu else torch.device('cpu')
    g = Graph(data_root=args.data_root, **hparams["graph"])
    if reduction is not None:                       # before the banner: its statistics are the reduced content's
        from .reduce import ContentPCA
        original_width = int(g.X.shape[1]) if sparse_content is None else int(sparse_content.shape[1])
        if arrivals is not None and arrivals[1].shape[1] != original_width:
            raise ValueError(f"new_vertices: with content_reduction the arrivals' content must have the graph's ORIGINAL "
                             f"width {original_width} (it is reduced to {reduction['dim'] or 'the loaded width'} by the "
                             f"graph's transform), got {tuple(arrivals[1].shape)}")
        if reduction_file is not None:
            loaded = ContentPCA.load(reduction_file)
            if reduction["dim"] is not None and reduction["dim"] != loaded.dim:
                raise ValueError(f"content_reduction: dim = {reduction['dim']} but {str(reduction_file)!r} reduces to "
                                 f"{loaded.dim} columns")
            if loaded.components_.shape[1] != original_width:
                raise ValueError(f"content_reduction: {str(reduction_file)!r} was fitted on {loaded.components_.shape[1]} "
                                 f"columns, the content has {original_width}")
            if sparse_content is not None:
                g.reduce_sparse_content(sparse_content, loaded.dim, transform=loaded)
            else:
                g.reduce_content(loaded.dim, transform=loaded)
        elif sparse_content is not None:
            g.reduce_sparse_content(sparse_content, reduction["dim"], center=reduction["center"],
                                    whiten=reduction["whiten"], oversample=reduction["oversample"],
                                    power_iterations=reduction["power_iterations"], seed=reduction["seed"])
        else:
            g.reduce_content(reduction["dim"], center=reduction["center"], whiten=reduction["whiten"])
        if arrivals is not None:                    # the graph's mean and components, never a re-fit
            arrivals = (arrivals[0], g.content_transform.transform(arrivals[1].to(g.X.dtype).contiguous()), *arrivals[2:])
    if arrivals is not None and arrivals[1].shape[1] != g.d:       # the one check that needs the graph: before any sweep
        raise ValueError(f"new_vertices: content must be [{len(arrivals[0])}, {g.d}], got {tuple(arrivals[1].shape)}")

    if world > 1:                                   # unseeded N(0,1) content (no C.npy) must agree across ranks
        import torch.distributed as dist
        Xd = g.X.cuda()
        dist.broadcast(Xd, 0)
        g.X = Xd.cpu()

    say("Graph Loaded.")
    say(f" - {len(g)} vertices")
    say(f" - {len(g.E)} edges")
    if reduction is not None and g.content_transform.sparse_fit_ is not None:
        fit = g.content_transform.sparse_fit_
        say(f" - Content Embeddings (reduced from {original_width} sparse columns, {fit['nnz']} non-zeros; method: "
            f"randomized, oversample {fit['oversample']}, power_iterations {fit['power_iterations']}, seed {fit['seed']}; "
            f"{g.content_transform.explained_variance_ratio_.sum():.3f} of the variance kept):")
    elif reduction is not None:
        say(f" - Content Embeddings (reduced from {original_width} columns; "
            f"{g.content_transform.explained_variance_ratio_.sum():.3f} of the variance kept):")
    else:
        say(" - Content Embeddings:")
    say(f"     - dim : {g.d:3d}")
    say(f"     - mean: {g.X.mean():5.2f}")
    say(f"     - std : {g.X.std():5.2f}")

    try:
        similarity_measure = getattr(similarity, hparams["similarity"]["method"])
    except AttributeError:
        raise AttributeError(f'Given similarity method {hparams["similarity"]["method"]} not found.')

    similarity_measure = similarity_measure(**hparams['similarity']['kwargs'])

    embedder_cls = IterativeEmbedder if hasattr(similarity_measure, 'parameters') else Embedder
    if embedder_cls is IterativeEmbedder and getattr(args, "train_similarity", False):
        if world > 1:
            raise NotImplementedError("--train_similarity runs on one GPU only; several GPUs are out of scope")
        embedder_cls = AlternatingEmbedder          # trains on the GPU, alternating with propagation
    extra = {"num_workers": args.num_workers} if embedder_cls is not Embedder else {}
    if world > 1 and getattr(args, "exchange", "auto") != "auto":
        g.engine(device if device.type == "cuda" else None, exchange=args.exchange)     # first use fixes the division
    if args.init_Z is not None:                     # resume: start from saved embeddings instead of Z = X
        Z0 = torch.from_numpy(np.load(args.init_Z))
        if tuple(Z0.shape) != tuple(g.X.shape):
            raise ValueError(f"--init_Z holds shape {tuple(Z0.shape)}, the graph needs {tuple(g.X.shape)}")
        g.set_Z(Z0.to(g.X.dtype))
    if args.save_history and embedder_cls is Embedder:
        # write output_root/{outer}/Z_{sweep}.npy (the reference's layout, __main__.py:73-86) WHILE the sweeps run
        def write_sweep(outer, sweep, Z):
            if rank == 0:
                folder = args.output_root.joinpath(f'{outer}')
                folder.mkdir(parents=True, exist_ok=True)
                np.save(folder.joinpath(f'Z_{sweep}.npy'), _to_numpy(Z))
        extra["history_sink"] = write_sweep
        if world > 1:       # every rank stages its own part of Z; rank 0's writer thread assembles them (one box: same disk)
            extra["history_parts_dir"] = args.output_root.joinpath(".clane_history_parts")
    embedder = embedder_cls(graph=g, similarity_measure=similarity_measure, device=device,
                            save_history=args.save_history, **extra, **hparams["embedder"])
    if rank != 0:
        embedder.verbose = False
    embedder.iterate()
    final_Z = g.Z                                   # collective when world > 1: every rank takes part
    if "history_parts_dir" in extra and rank == 0:
        shutil.rmtree(extra["history_parts_dir"], ignore_errors=True)      # iterate() flushed: every part was consumed
    if world > 1:                                   # leave together: nobody tears the group down while others talk
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if rank != 0:
        return

    say("Saving the results.")
    if not args.output_root.exists():
        args.output_root.mkdir(parents=True, exist_ok=True)

    np.save(args.output_root.joinpath('Z.npy'), _to_numpy(final_Z))

    say(f"The embeddings are stored in {args.output_root.joinpath('Z.npy').absolute()}.")

    if reduction is not None:
        import json
        g.content_transform.save(args.output_root.joinpath('content_projection.npz'))
        with open(args.output_root.joinpath('content_reduction.json'), "w") as io:
            json.dump(g.content_transform.report(original_width), io, indent=1)
            io.write("\n")
        say(f"The content projection ({original_width} -> {g.d} columns) is stored in "
            f"{args.output_root.joinpath('content_projection.npz').absolute()}.")

    if predict_k is not None:
        from .links import read_link_sources, write_links_tsv
        sources = None if args.link_sources is None else read_link_sources(args.link_sources, g.vertex_ids)
        ids, scores = g.predict_links(similarity_measure, k=predict_k, sources=sources)
        n = write_links_tsv(args.output_root.joinpath('links.tsv'), g.vertex_ids, sources, ids, scores)
        say(f"{n} predicted links are stored in {args.output_root.joinpath('links.tsv').absolute()}.")

    if link_eval is not None:                       # with the similarity the run ends with: trained weights included
        import json
        from .links import read_link_pairs
        pairs_file = Path(link_eval["pairs"])
        if not pairs_file.is_absolute():
            pairs_file = Path(args.data_root) / pairs_file
        src, dst = read_link_pairs(pairs_file, g.vertex_ids)
        filtered = bool(link_eval.get("filter_existing", True))
        metrics = g.evaluate_links(similarity_measure, src, dst, hits=tuple(link_eval.get("hits", (1, 3, 10))),
                                   filter_existing=filtered)
        out = args.output_root.joinpath('link_metrics.json')
        with open(out, "w") as io:
            json.dump({**metrics, "similarity": type(similarity_measure).__name__, "filtered": filtered}, io, indent=1)
            io.write("\n")
        say(f"The link metrics of {metrics['pairs']} held-out pairs are stored in {out.absolute()}.")

    if node_cls is not None:                        # the README's experiment on the embeddings the run ends with
        import json
        labels_file = Path(node_cls["labels"])
        if not labels_file.is_absolute():
            labels_file = Path(args.data_root) / labels_file
        kw = {key: node_cls[key] for key in ("ratios", "runs", "seed", "l2", "multilabel", "predict") if key in node_cls}
        if not kw.get("multilabel", False):
            kw.pop("multilabel", None)
        tables = {"Z": g.evaluate_labels(labels_file, table="Z", **kw)}
        if node_cls.get("baseline", False):
            tables["X"] = g.evaluate_labels(labels_file, table="X", **kw)
        first = tables["Z"]
        out = args.output_root.joinpath('label_metrics.json')
        with open(out, "w") as io:
            json.dump({"labels": str(labels_file), "labelled": first["labelled"], "class_names": first["class_names"],
                       "ratios": [r["ratio"] for r in first["rows"]], "runs": first["runs"], "seed": first["seed"],
                       "l2": first["l2"],
                       **({"multilabel": True, "predict": first["predict"],
                           "constant_columns": {name: t["constant_columns"] for name, t in tables.items()}}
                          if first.get("multilabel") else {}),
                       "tables": {name: {"rows": t["rows"], "fits": t["fits"], "skipped_fits": t["skipped_fits"]}
                                  for name, t in tables.items()}}, io, indent=1)
            io.write("\n")
        say(f"The F1 table of {first['labelled']} labelled vertices is stored in {out.absolute()}.")

    label_model = label_report = None
    if label_pred is not None:                      # a kept classifier on the embeddings the run ends with
        from . import classify
        label_model, label_report = classify.run_section(label_pred, g, args.output_root)
        classify.write_report(args.output_root, label_report)       # written again below with the arrivals' count
        say(f"The predicted labels of {label_report['predicted']} vertices ({label_report['model']} model, l2 = "
            f"{label_report['l2']}) are stored in {args.output_root.joinpath('predicted_labels.tsv').absolute()}.")

    if node_clu is not None:                        # k-means on the embeddings the run ends with
        import json
        labels_file = None
        if "labels" in node_clu:
            labels_file = Path(node_clu["labels"])
            if not labels_file.is_absolute():
                labels_file = Path(args.data_root) / labels_file
        kw = {key: node_clu[key] for key in ("restarts", "seed", "max_iter") if key in node_clu}
        kw.update(k=node_clu.get("clusters"), labels=labels_file, return_assignments=True, **node_clu_scoring)
        tables = {"Z": g.cluster(table="Z", **kw)}
        if node_clu.get("baseline", False):
            tables["X"] = g.cluster(table="X", **kw)
        first = tables["Z"]
        hidden = ("vertices", "assignments", "class_names", "table", "clustered", "clusters", "restarts", "seed")
        out = args.output_root.joinpath('cluster_metrics.json')
        with open(out, "w") as io:
            json.dump({"labels": None if labels_file is None else str(labels_file), "clustered": first["clustered"],
                       "class_names": first.get("class_names"), "clusters": first["clusters"],
                       "restarts": first["restarts"], "seed": first["seed"],
                       "tables": {name: {key: v for key, v in t.items() if key not in hidden}
                                  for name, t in tables.items()}}, io, indent=1)
            io.write("\n")
        if node_clu.get("assignments", False):
            with open(args.output_root.joinpath('clusters.tsv'), "w") as io:
                for v, c in zip(first["vertices"], first["assignments"]):
                    io.write(f"{g.vertex_ids[v]}\t{c}\n")
        say(f"The clustering of {first['clustered']} vertices into {first['clusters']} clusters is stored in "
            f"{out.absolute()}.")

    mixture_model = mixture_report = None
    if soft_clu is not None:                        # a Gaussian mixture on the embeddings the run ends with
        from . import mixture
        mixture_model, mixture_report = mixture.run_section(soft_clu, g, args.output_root)
        mixture.write_report(args.output_root, mixture_report)      # written again below with the arrivals' count
        say(f"The soft clustering of {mixture_report['clustered']} vertices into {mixture_report['clusters']} components "
            f"is stored in {args.output_root.joinpath('mixture_metrics.json').absolute()}.")

    if layout_cfg is not None:                      # the picture of the embeddings the run ends with
        from . import layout as layout_mod
        kw = {key: layout_cfg[key] for key in ("perplexity", "max_points", "max_iter", "seed", "method", "neighbours")
              if key in layout_cfg}
        tables = {"Z": g.layout(table="Z", labels=layout_labels, **kw)}
        if layout_cfg["baseline"]:
            tables["X"] = g.layout(table="X", labels=layout_labels, **kw)
        report = layout_mod.write_results(args.output_root, g.vertex_ids, tables)
        say(f"The 2-D layout of {report['n']} vertices ({report['iterations']} iterations, KL {report['kl']:.4f}) is "
            f"stored in {args.output_root.joinpath('layout.tsv').absolute()}.")

    if arrivals is not None:                        # with the similarity the run ends with: trained weights included
        from . import induct
        new_ids, X_new, rowptr, cols = arrivals
        emb = hparams.get("embedder") or {}
        res = g.embed_new(similarity_measure, X_new, (rowptr, cols), gamma=emb.get("gamma", 0.76),
                          tolerence=emb.get("tolerence", 10), max_rounds=new_vertices["max_rounds"],
                          weights=new_vertices["weights"])
        report = induct.write_results(args.output_root, new_ids, g.vertex_ids, res, similarity_measure,
                                      new_vertices["max_rounds"], new_vertices["weights"])
        say(f"The embeddings of {report['new_vertices']} new vertices ({report['not_converged']} not converged) are "
            f"stored in {args.output_root.joinpath('Z_new.npy').absolute()}.")
        if label_model is not None:                 # the same model on the arrivals, in the order of their V
            from . import classify
            eng = g.engine()
            classes, probs = label_model.predict_rows(eng, res.Z.to(eng.device, eng.Zcur.dtype).contiguous(),
                                                      top=label_pred["top"])
            label_report["predicted_new"] = classify.write_predictions_tsv(
                args.output_root.joinpath('predicted_labels_new.tsv'), new_ids, label_model.class_names, classes, probs)
            classify.write_report(args.output_root, label_report)
        if mixture_model is not None:               # the same mixture on the arrivals, in the order of their V
            from . import mixture
            eng = g.engine()
            comp, prob = mixture_model.predict_rows(eng, res.Z.to(eng.device, eng.Zcur.dtype).contiguous(),
                                                    top=soft_clu["top"])
            mixture_report["assigned_new"] = mixture.write_memberships_tsv(
                args.output_root.joinpath('memberships_new.tsv'), new_ids, comp, prob)
            mixture.write_report(args.output_root, mixture_report)


def _to_numpy(Z: torch.Tensor) -> np.ndarray:
    Z = Z.cpu()
    return (Z.float() if Z.dtype == torch.bfloat16 else Z).numpy()      # NumPy has no bfloat16


def get_parser():
    parser = argparse.ArgumentParser(prog="clane")
    parser.add_argument("command", nargs="?", choices=["embedding"], default="embedding",
                        help="Optional; the only command is 'embedding'.")
    parser.add_argument("--data_root", type=Path, help="Path to the data root directory.")
    parser.add_argument("--output_root", type=Path, help="Path to the root for the experiment results to be stored.")
    parser.add_argument("--config_file", type=Path, help="Path to the training configuration yaml file.")
    parser.add_argument("--save_history", action='store_true',
                        help="If true, it saves the embeddings for every iteration.")
    parser.add_argument("--num_workers", type=int, default=0)
    parser.add_argument("--init_Z", type=Path, default=None,
                        help="(extension) .npy of shape [V, d]: start from these embeddings instead of the content "
                             "embeddings, e.g. the Z.npy of an interrupted run.")
    parser.add_argument("--exchange", default="auto",
                        choices=["auto", "columns", "allgather_all", "allgather", "halo", "halo_p2p"],
                        help="(extension, multi-GPU runs under torchrun) how the sweep is divided over the GPUs: columns of "
                             "Z (no exchange per sweep; what auto picks for wide rows), rows with one all-gather of the "
                             "updated rows per sweep (allgather_all) or the leaner row splits; "
                             "see DESIGN.md section 6.  A plug-in similarity needs a row division (default then: halo).")
    parser.add_argument("--train_similarity", action='store_true',
                        help="(extension) with a similarity that has parameters (AsymmertricSimilarity): train it on the "
                             "GPU, alternating with propagation (AlternatingEmbedder; the config's embedder keys are the "
                             "reference's: tolerence, tolerence_Z, tolerence_P, epoch, batch_size, lr).  One GPU only.  "
                             "Without the flag such a config ends as before: IterativeEmbedder is not implemented.")
    parser.add_argument("--predict_links", type=int, default=None, metavar="K",
                        help="(extension) after the embedding, write output_root/links.tsv: for every vertex the K (1..32) "
                             "vertices it is most likely to link to under the configured similarity and does not link to "
                             "yet, one 'src_id<TAB>dst_id<TAB>score' line per candidate, best first.  CosineSimilarity "
                             "and AsymmertricSimilarity; one GPU only.")
    parser.add_argument("--link_sources", type=Path, default=None, metavar="FILE",
                        help="(extension) with --predict_links: a file of vertex ids, one per line -- rank links for these "
                             "sources only, in the file's order.")
    parser.add_argument("--gpu", action='store_true')
    return parser


def main():
    parser = get_parser()
    args = parser.parse_args()
    embedding(args)


if __name__ == "__main__":
    main()
