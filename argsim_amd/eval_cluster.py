#!/usr/bin/env python3
"""downstream clustering of the embeddings on the device (counterpart of reference src/eval_clustering.py:82-103 and, with --by all,
src/eval_clustering_explorative.py:138-176): Ward agglomerative clustering per selection of rows, as many clusters as the selection
has distinct `topic-stance-reason` labels, scored by the adjusted Rand score and the V-measure.  Every selection of a run is one
group of ONE device call (VAE.cluster_eval).  Prints the reference's lines.

    python -m argsim_amd.eval_cluster --inputs data/test_data_emb.npy --labels data/test_labels.npy --by stance

--by topic | stance | reason: one selection per topic, per (topic, stance) or per (topic, reason), in sorted order
(eval_clustering.py:86-92, where the partition picked at its line 35 decides).  --by all: the whole set cut at the number of topics
and at the number of labels, then every topic's rows against their labels.  --dims: an .npy of column numbers to keep (the
useful_dimension.npy that eval_clustering.py:57-58 writes).  --select topic | stance | reason | labels: pick those columns here instead,
as eval_clustering.py:46-58 does -- the L1 logistic model (C = 0.1) of that partition of the labels, fitted on the device
(VAE.select_dims; the reference's line 35 picks stance), keeping the columns with a nonzero coefficient in any class -- print how many
were kept, write them with --save-dims PATH, and cluster on them."""
import argparse

import numpy as np

LINE = "{:<20s}\tARS: {:.4F}\tV_MSR: {:.4f}"


def split_labels(labels):
    """-> (topics, full): the topic of every row and its (topic, stance, reason) as one string key"""
    parts = [tuple(str(label).split("-")) for label in labels]
    for p in parts:
        if len(p) != 3:
            raise ValueError("labels are topic-stance-reason strings, got %r" % ("-".join(p),))
    return parts


def selections(parts, by):
    """eval_clustering.py:86-92 -> {selection: row numbers}, in sorted order of the selections"""
    pick = {'topic': lambda p: p[0], 'stance': lambda p: (p[0], p[1]), 'reason': lambda p: (p[0], p[2])}[by]
    keys = [pick(p) for p in parts]
    return {sel: np.array([i for i, k in enumerate(keys) if k == sel]) for sel in sorted(set(keys))}


def report(scores):
    return [LINE.format(str(sel), ars, v) for sel, (ars, v) in scores.items()]


def report_all(scores, topics):
    """the lines of eval_clustering_explorative.py:144,155,176"""
    lines = ["TOPIC:  ARS: {:.4F}\tV_MSR: {:.4f}".format(*scores['TOPIC']), "REASON: ARS: {:.4F}\tV_MSR: {:.4f}".format(*scores['REASON'])]
    return lines + ["{:<20s}: ARS: {:.4F}\tV_MSR: {:.4f}".format(t, *scores[('topic', t)]) for t in topics]


def evaluate(vae, z, labels, by):
    """-> (scores, lines)"""
    from . import cluster
    parts = split_labels(labels)
    full = np.array(["-".join(p) for p in parts])
    if by != 'all':
        scores = vae.cluster_eval(z, full, selections(parts, by))
        return scores, report(scores)
    topics = np.array([p[0] for p in parts])
    order = list(dict.fromkeys(topics.tolist()))
    groups = {'ALL': np.arange(len(parts))}
    groups.update({('topic', t): np.flatnonzero(topics == t) for t in order})
    res = vae.ward(z, groups)
    k = {key: len(np.unique(full[res['groups'][key]['rows']])) for key in res['keys']}
    by_label = vae.ward_cut(res, k)
    k['ALL'] = len(order)
    by_topic = vae.ward_cut(res, k)
    score = lambda gold, pred: (cluster.adjusted_rand(gold, pred), cluster.v_measure(gold, pred))
    scores = {'TOPIC': score(topics, by_topic['ALL']), 'REASON': score(full, by_label['ALL'])}
    for t in order:
        scores[('topic', t)] = score(full[groups[('topic', t)]], by_label[('topic', t)])
    return scores, report_all(scores, order)


def partition(parts, which):
    """the gold partition of eval_clustering.py:16-35 -> (n,) strings: the topic, (topic, stance), (topic, reason) or the whole label"""
    pick = {'topic': lambda p: p[0], 'stance': lambda p: p[0] + '-' + p[1], 'reason': lambda p: p[0] + '-' + p[2], 'labels': "-".join}[which]
    return np.array([pick(p) for p in parts])


def select(vae, z, labels, which, C=0.1):
    """eval_clustering.py:46-58 on the device: the columns of z that the L1 model of that partition uses -> dims (int64, sorted)"""
    dims, probe = vae.select_dims(z, partition(split_labels(labels), which), C=C)
    if probe.stats.shape[0] and (probe.stats[:, 3] != 0).any():
        raise RuntimeError("the L1 fit of the selection did not converge: status %s per class" % (probe.stats[:, 3].astype(int).tolist(),))
    if dims.shape[0] == 0:
        raise RuntimeError("the selection keeps no column: every coefficient of the L1 model at C = %g is zero" % C)
    return dims


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--inputs', required=True, help=".npy (n, dim) float32 embeddings (eval_embed's output)")
    ap.add_argument('--labels', required=True, help=".npy (n,) strings topic-stance-reason")
    ap.add_argument('--by', choices=('topic', 'stance', 'reason', 'all'), default='stance')
    which = ap.add_mutually_exclusive_group()
    which.add_argument('--dims', default=None, help=".npy of the column numbers to cluster on (useful_dimension.npy)")
    which.add_argument('--select', choices=('topic', 'stance', 'reason', 'labels'), default=None,
                       help="pick the columns on the device: those the L1 model (C = 0.1) of this partition of the labels uses")
    ap.add_argument('--save-dims', default=None, help="with --select: write the kept column numbers to this .npy (int64)")
    ap.add_argument('--device', type=int, default=0)
    return ap


def main(argv=None):
    ap = build_parser()
    A = ap.parse_args(argv)
    if A.save_dims is not None and A.select is None:
        ap.error("--save-dims needs --select")
    z = np.load(A.inputs)
    labels = np.load(A.labels)
    vae = make_vae(A.device)
    if A.dims is not None:
        z = z[:, np.load(A.dims)]
    elif A.select is not None:
        dims = select(vae, np.ascontiguousarray(z, dtype=np.float32), labels, A.select)
        print("useful dimensions: %d of %d" % (dims.shape[0], z.shape[1]))
        if A.save_dims is not None:
            np.save(A.save_dims, dims)
        z = z[:, dims]
    z = np.ascontiguousarray(z, dtype=np.float32)
    scores, lines = evaluate(vae, z, labels, A.by)
    for line in lines:
        print(line)
    return scores


def make_vae(device):
    # the clustering does not use the model: any handle serves
    from .model import VAE
    return VAE('infer', device=device, init=False, dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)


if __name__ == '__main__':
    main()
