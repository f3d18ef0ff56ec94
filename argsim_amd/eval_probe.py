#!/usr/bin/env python3
"""downstream classification of the embeddings on the device (counterpart of reference src/eval_classification.py and, with
--stance, src/eval_classification_stance.py): a one-vs-rest L2 logistic regression (liblinear's model, C = 0.001, balanced class
weights) per topic, scored by cross-validation over the given folds -- every topic x fold x class of a run is one problem of ONE
batched fit (VAE.probe_cv).  Prints `topic score` lines and the mean over the topics, in the reference's format.

    python -m argsim_amd.eval_probe --inputs data/test_data_emb.npy --labels data/test_labels.npy --folds data/test_folds.npy

Labels are `topic-stance-reason` strings: the group is the topic and the class is `stance-reason`.  --stance: the class is the
stance (C = 0.1), preceded by one line with the score of classifying the topic over all rows (C = 0.01)."""
import argparse

import numpy as np


def split_labels(labels, stance=False):
    """-> (topics, classes): eval_classification.py:23-27, or with stance the top / stn arrays of eval_classification_stance.py"""
    topics, classes = [], []
    for label in labels:
        topic, st, reason = str(label).split("-")
        topics.append(topic)
        classes.append(st if stance else "{}-{}".format(st, reason))
    return np.array(topics), np.array(classes)


def report(res):
    """the reference's output: one `topic score` line per topic (two decimals of the percentage) and the mean of the raw scores"""
    lines = ["{} {:.2f}".format(t, s * 100) for t, s in res['scores'].items()]
    return lines + [str(np.mean(list(res['scores'].values())))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--inputs', required=True, help=".npy (n, dim) float32 embeddings (eval_embed's output)")
    ap.add_argument('--labels', required=True, help=".npy (n,) strings topic-stance-reason")
    ap.add_argument('--folds', required=True, help=".npy (n,) fold of every row")
    ap.add_argument('--stance', action='store_true')
    ap.add_argument('--cost', type=float, default=None, help="C (default 0.001; with --stance 0.1)")
    ap.add_argument('--tol', type=float, default=None)
    ap.add_argument('--device', type=int, default=0)
    A = ap.parse_args(argv)
    from . import probe
    from .model import VAE
    z = np.ascontiguousarray(np.load(A.inputs), dtype=np.float32)
    topics, classes = split_labels(np.load(A.labels), A.stance)
    folds = np.load(A.folds)
    # the probes do not use the model: any handle serves
    vae = VAE('infer', device=A.device, init=False, dim_tgt=32, dim_emb=16, dim_rep=8, rnn_layers=1)
    solver = dict(tol=probe.DEFAULT_TOL if A.tol is None else A.tol)
    if A.stance:
        print(vae.probe_cv(z, topics, folds, None, C=0.01, **solver)['mean'])
    cost = A.cost if A.cost is not None else (0.1 if A.stance else 0.001)
    res = vae.probe_cv(z, classes, folds, topics, C=cost, **solver)
    bad = int((res['stats'][:, 3] != 0).sum())
    for line in report(res):
        print(line)
    if bad:
        print("warning: %d of %d problems did not converge" % (bad, res['stats'].shape[0]))
    return res


if __name__ == '__main__':
    main()
