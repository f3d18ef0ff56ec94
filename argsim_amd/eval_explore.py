#!/usr/bin/env python3
"""explorative clustering of the embeddings on the device (counterpart of reference src/eval_clustering_explorative.py:69-132):
affinity propagation over all rows on Euclidean and on cosine similarities, for the embeddings and, where given, for the embeddings
of the sampled segmentation; per run the topics' purity listing and the cluster count, then every row's distance to its cluster
centroid, written with the cluster numbers as CSV.  Every run is ONE device call (VAE.affinity).

    python -m argsim_amd.eval_explore --inputs data/test_data_emb.npy --labels data/test_labels.npy \\
        [--inputs-sp data/test_data_emb_sample.npy] [--posts data/test_posts.npy] [--csv trial/clustering.csv]
        [--tsne trial/tsne.npy [--tsne-plot trial/tsne.png] [--perplexity 40] [--tsne-iter 20000]] [--kmeans K [--kmeans-init 10]]
        [--quality] [--sweep LO:HI[:STEP]] [--gmm K [--gmm-cov diag|spherical] [--gmm-init R]] [--gmm-sweep LO:HI[:STEP]]
        [--dbscan EPS [--dbscan-min M]] [--dbscan-sweep E1,E2,..] [--pca K [--pca-whiten]] [--mmd stance [--mmd-perm P]]

With --tsne the script first does what lines 45-66 of the reference do: the exact t-SNE of the embeddings into two dimensions in ONE
device call (VAE.tsne, a random start as in the reference's sklearn), written as .npy and, with --tsne-plot, scattered by topic.

The labels are eval_cluster's topic-stance-reason strings; the topics are listed in order of first appearance.  A purity line is the
topic, then share|members|cluster for the clusters of which at least half the members (and at least two) belong to the topic.

With --kmeans K the same runs follow with k-means into K clusters (VAE.kmeans: k-means++ seeding, the best of --kmeans-init restarts, ONE
device call each), the same lines per run and the columns cls_km_* / dist_km_* in the CSV.  Without it nothing changes.

With --quality every run that was made is followed by one line "silhouette %.4f  CH %.2f  DB %.4f": the silhouette score, the
Calinski-Harabasz and the Davies-Bouldin index of its clusters on its own metric (VAE.silhouette, ONE device call).  With --sweep LO:HI[:STEP]
the table "k silhouette CH DB" of k-means for every k of the range follows per input and metric (VAE.sweep_k: one k-means call per k, ONE
silhouette call over all of them), the k with the largest silhouette marked with *.  Without the two flags the output is what it was.

With --gmm K a Gaussian mixture with K components is fitted to the embeddings and, where given, to those of the sampled segmentation
(VAE.gmm: --gmm-cov covariances, the best of --gmm-init restarts from k-means labels, ONE device call each after the k-means calls): the
same lines per run for its hard labels, and the columns cls_gmm_* / logp_gmm_* (a row's component and its log-density) in the CSV.  With
--gmm-sweep LO:HI[:STEP] the table "k BIC AIC lower_bound" follows per input (VAE.sweep_gmm), the k with the smallest BIC marked with *.
Without these flags the output is what it was.

With --dbscan EPS the same runs follow with density clustering (VAE.dbscan: --dbscan-min rows within EPS make a row core, ONE device call
each; no cluster count, rows of no cluster are noise): the purity lines over the clustered rows, "N clusters, M noise rows", with --quality
the scores over the clustered rows, and the columns cls_db_* / dist_db_* in the CSV (noise: -1 and nan).  With --dbscan-sweep E1,E2,.. the
table "eps clusters noise silhouette CH DB" follows per input and metric (VAE.sweep_eps: one dbscan call per eps, ONE silhouette call over
all that can be scored), the eps with the largest silhouette marked with *.  Without these flags the output is what it was.

With --pca K (a count, or a fraction in (0, 1) of the variance to keep) the embeddings and, where given, those of the sampled segmentation
are first reduced to their leading principal components (VAE.pca_reduce: ONE device call for the fit, one for the projection; --pca-whiten
scales them to unit variance): per input the table "component variance ratio cumulative" and the line "effective dimension %.2f of D,
rank R, kept K", and EVERY run above is made on the reduced rows.  Without the flag nothing changes.

With --mmd stance the table "topic m n mmd2 p" follows per input: per topic, do the rows of its first stance and those of its second come
from the same distribution?  The kernel two-sample test (VAE.mmd: the rbf kernel at the median bandwidth, --mmd-perm relabelings, all
topics in ONE device call); a topic with fewer than two rows of either stance is listed as n/a.  Without the flag nothing changes."""
import argparse
import csv

import numpy as np

RUNS = (('euc', 'euclidean', 'sqeuclidean', False), ('euc_sp', 'euclidean', 'sqeuclidean', True), ('cos', 'cosine', 'cosine', False),
        ('cos_sp', 'cosine', 'cosine', True))
COLUMNS = "post topic labels cls_euc dist_euc cls_euc_sp dist_euc_sp cls_cos dist_cos cls_cos_sp dist_cos_sp".split()
KM_COLUMNS = "cls_km_euc dist_km_euc cls_km_euc_sp dist_km_euc_sp cls_km_cos dist_km_cos cls_km_cos_sp dist_km_cos_sp".split()      # with --kmeans
DB_COLUMNS = "cls_db_euc dist_db_euc cls_db_euc_sp dist_db_euc_sp cls_db_cos dist_db_cos cls_db_cos_sp dist_db_cos_sp".split()      # with --dbscan
GMM_RUNS = (('z', False), ('z_sp', True))
GMM_COLUMNS = "cls_gmm_z logp_gmm_z cls_gmm_z_sp logp_gmm_z_sp".split()      # with --gmm


def purity_lines(pred, topics, order):
    """the lines of eval_clustering_explorative.py:77-81 for one run"""
    from . import affinity
    lines = []
    for topic in order:
        cells = ["{:.3f}|{:03d}|{:03d}".format(acc, n, c) for c, n, acc in affinity.purity(pred, topics == topic)]
        lines.append(" ".join([topic.ljust(9)] + cells))
    return lines + ["%d clusters" % len(set(np.asarray(pred).tolist()))]


def quality_line(vae, x, pred, metric):
    """the line of --quality for one run; a run with one cluster, or with as many as rows, has no scores"""
    try:
        q = vae.silhouette(x, np.asarray(pred, np.int64), metric)
    except ValueError:
        return "silhouette n/a (%d clusters)" % len(set(np.asarray(pred).tolist()))
    return "silhouette %.4f  CH %.2f  DB %.4f" % (q['score'], q['ch'], q['db'])


def sweep_lines(vae, x, name, metric, ks, n_init, seed):
    """the table of --sweep for one input and metric"""
    t = vae.sweep_k(x, ks, metric, n_init=n_init, seed=seed)
    lines = ["sweep %s" % name, "k silhouette CH DB"]
    for k, s, ch, db in zip(t['k'], t['score'], t['ch'], t['db']):
        lines.append("%d %.4f %.2f %.4f%s" % (k, s, ch, db, " *" if k == t['best'] else ""))
    return lines


def gmm_sweep_lines(vae, x, name, ks, covariance, n_init, seed):
    """the table of --gmm-sweep for one input"""
    t = vae.sweep_gmm(x, ks, covariance=covariance, n_init=n_init, seed=seed)
    lines = ["gmm sweep %s" % name, "k BIC AIC lower_bound"]
    for k, bic, aic, lb in zip(t['k'], t['bic'], t['aic'], t['lower_bound']):
        lines.append("%d %.2f %.2f %.6f%s" % (k, bic, aic, lb, " *" if k == t['best'] else ""))
    return lines


def dbscan_lines(res, topics, order):
    """the lines of --dbscan for one run: the purity listing over the rows that are in a cluster, then the counts"""
    on = res['labels'] >= 0
    lines = purity_lines(res['labels'][on], topics[on], order)[:-1] if on.any() else []
    return lines + ["%d clusters, %d noise rows" % (res['n_clusters'], res['n_noise'])]


def eps_sweep_lines(vae, x, name, metric, eps_list, min_samples):
    """the table of --dbscan-sweep for one input and metric"""
    t = vae.sweep_eps(x, eps_list, min_samples, metric)
    lines = ["dbscan sweep %s" % name, "eps clusters noise silhouette CH DB"]
    for e, k, n, s, ch, db in zip(t['eps'], t['n_clusters'], t['n_noise'], t['score'], t['ch'], t['db']):
        lines.append("%g %d %d %.4f %.2f %.4f%s" % (e, k, n, s, ch, db, " *" if t['best'] is not None and e == t['best'] else ""))
    return lines


def pca_lines(model, name):
    """the table of --pca for one input"""
    lines = ["pca %s" % name, "component variance ratio cumulative"]
    cum = np.cumsum(model['explained_variance_ratio'])
    for c, (v, r, s) in enumerate(zip(model['explained_variance'], model['explained_variance_ratio'], cum)):
        lines.append("%d %.6g %.4f %.4f" % (c, v, r, s))
    return lines + ["effective dimension %.2f of %d, rank %d, kept %d" % (model['effective_dim'], len(model['mean']), model['rank'],
                                                                           len(model['explained_variance']))]


def mmd_lines(vae, x, name, labels, n_perm, seed):
    """the table of --mmd stance for one input: per topic its first stance (A) against its second (B)"""
    from .eval_cluster import split_labels
    parts = split_labels(labels)
    topics, stances = np.array([p[0] for p in parts]), np.array([p[1] for p in parts])
    lines = ["mmd stance %s" % name, "topic m n mmd2 p"]
    rows, names = [], []
    for topic in dict.fromkeys(topics.tolist()):
        on = topics == topic
        kinds = list(dict.fromkeys(stances[on].tolist()))[:2]
        g = np.full(len(topics), -1, np.int64)
        for side, kind in enumerate(kinds):
            g[on & (stances == kind)] = side
        if min(int((g == 0).sum()), int((g == 1).sum())) < 2:
            lines.append("%s %d %d n/a" % (topic, int((g == 0).sum()), int((g == 1).sum())))
        else:
            rows.append(g)
            names.append(topic)
    for i0 in range(0, len(rows), 64):
        t = vae.mmd(x, np.stack(rows[i0:i0 + 64]), n_perm=n_perm, seed=seed)
        for topic, m, n, s, p in zip(names[i0:i0 + 64], t['m'], t['n'], t['stat'], t['pvalue']):
            lines.append("%s %d %d %.6f %.4f" % (topic, m, n, s, p))
    return lines


def evaluate(vae, z, z_sp, labels, seed=0, max_iter=200, kmeans=None, kmeans_init=10, quality=False, sweep=None, gmm=None, gmm_cov='diag',
             gmm_init=1, gmm_sweep=None, dbscan=None, dbscan_min=5, dbscan_sweep=None, pca=None, pca_whiten=False, mmd=None, mmd_perm=999):
    """-> (columns {name: array}, lines): cls_* / dist_* of the runs that have their inputs, and what is printed.  kmeans = k adds the
    same runs with k-means into k clusters (VAE.kmeans, kmeans_init restarts): cls_km_* / dist_km_*.  quality: a line of scores behind
    every run; sweep = [k ..]: the k-means quality table per input and metric.  gmm = k adds a mixture with k components per input
    (VAE.gmm, gmm_cov covariances, gmm_init restarts): cls_gmm_* / logp_gmm_*; gmm_sweep = [k ..]: the BIC / AIC table per input.
    dbscan = eps adds the same runs with density clustering (VAE.dbscan, dbscan_min rows make a core row): cls_db_* / dist_db_*;
    dbscan_sweep = [eps ..]: the quality table per input and metric.  pca = k (a count or a fraction): every run is made on the rows
    reduced to their leading principal components (VAE.pca_reduce, pca_whiten: to unit variance), the variance table first.  mmd =
    'stance': per input the two-sample table of every topic's two stances (VAE.mmd, mmd_perm relabelings)"""
    from . import affinity
    from .eval_cluster import split_labels
    topics = np.array([p[0] for p in split_labels(labels)])
    order = list(dict.fromkeys(topics.tolist()))
    cols, lines = {}, []
    if pca:
        reduced = []
        for name, x in (('z', z), ('z_sp', z_sp)):
            if x is not None:
                x, model = vae.pca_reduce(x, pca, pca_whiten)
                lines += pca_lines(model, name)
            reduced.append(x)
        z, z_sp = reduced
    for name, metric, dist, sampled in RUNS:
        x = z_sp if sampled else z
        if x is None:
            continue
        res = vae.affinity(x, metric, max_iter=max_iter, seed=seed)
        if not res['converged']:
            lines.append("%s: did not converge in %d iterations" % (name, res['n_iter']))
        lines += purity_lines(res['labels'], topics, order)
        if quality:
            lines.append(quality_line(vae, x, res['labels'], metric))
        cols['cls_' + name] = res['labels']
        cols['dist_' + name] = affinity.dist_to_centroids(x, res['labels'], dist)
    for name, metric, dist, sampled in RUNS if kmeans else ():
        x = z_sp if sampled else z
        if x is None:
            continue
        res = vae.kmeans(x, kmeans, metric, n_init=kmeans_init, seed=seed)
        if res['stop'] == 'max_iter':
            lines.append("km_%s: stopped after %d iterations" % (name, res['n_iter']))
        lines += purity_lines(res['labels'], topics, order)
        if quality:
            lines.append(quality_line(vae, x, res['labels'], metric))
        cols['cls_km_' + name] = res['labels']
        cols['dist_km_' + name] = affinity.dist_to_centroids(x, res['labels'], dist)
    for name, metric, dist, sampled in RUNS if sweep else ():
        x = z_sp if sampled else z
        if x is not None:
            lines += sweep_lines(vae, x, name, metric, sweep, kmeans_init, seed)
    for name, sampled in GMM_RUNS if gmm else ():
        x = z_sp if sampled else z
        if x is None:
            continue
        res = vae.gmm(x, gmm, covariance=gmm_cov, n_init=gmm_init, seed=seed)
        if not res['converged']:
            lines.append("gmm_%s: stopped after %d iterations" % (name, res['n_iter']))
        lines += purity_lines(res['labels'], topics, order)
        lines.append("gmm_%s: lower bound %.6f  BIC %.2f  AIC %.2f" % (name, res['lower_bound'], res['bic'], res['aic']))
        cols['cls_gmm_' + name] = res['labels']
        cols['logp_gmm_' + name] = res['logp']
    for name, sampled in GMM_RUNS if gmm_sweep else ():
        x = z_sp if sampled else z
        if x is not None:
            lines += gmm_sweep_lines(vae, x, name, gmm_sweep, gmm_cov, gmm_init, seed)
    for name, metric, dist, sampled in RUNS if dbscan else ():
        x = z_sp if sampled else z
        if x is None:
            continue
        res = vae.dbscan(x, dbscan, dbscan_min, metric)
        lines += dbscan_lines(res, topics, order)
        if quality:
            lines.append(quality_line(vae, x, res['labels'], metric))
        cols['cls_db_' + name] = res['labels']
        cols['dist_db_' + name] = np.where(res['labels'] >= 0, affinity.dist_to_centroids(x, res['labels'], dist), np.nan)
    for name, metric, dist, sampled in RUNS if dbscan_sweep else ():
        x = z_sp if sampled else z
        if x is not None:
            lines += eps_sweep_lines(vae, x, name, metric, dbscan_sweep, dbscan_min)
    for name, sampled in GMM_RUNS if mmd == 'stance' else ():
        x = z_sp if sampled else z
        if x is not None:
            lines += mmd_lines(vae, x, name, labels, mmd_perm, seed)
    return cols, lines


def embed(vae, z, labels, out, plot=None, perplexity=40.0, max_iter=20000, seed=0):
    """eval_clustering_explorative.py:45-66 -> (the result of VAE.tsne, the line that is printed); the embedding goes to `out`"""
    from . import tsne
    from .eval_cluster import split_labels
    res = vae.tsne(z, perplexity=perplexity, max_iter=max_iter, init='random', seed=seed)
    np.save(out, res['y'])
    if plot:
        tsne.plot(plot, res['y'], [p[0] for p in split_labels(labels)])
    return res, "t-SNE: KL %.6f after %d iterations (%s)" % (res['kl'], res['n_iter'], res['stop'])


def write_csv(path, posts, topics, labels, cols):
    """eval_clustering_explorative.py:121-132: the id, then the columns in the reference's order (those of absent runs left out)"""
    names = [c for c in COLUMNS + KM_COLUMNS + GMM_COLUMNS + DB_COLUMNS if c in ('post', 'topic', 'labels') or c in cols]
    data = dict(cols, post=posts, topic=topics, labels=labels)
    with open(path, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['id'] + names)
        for i in range(len(labels)):
            w.writerow([i] + [data[c][i] for c in names])


def _positive(text):
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError("must be >= 1, got %r" % (text,))
    return v


def _sweep(text):
    """LO:HI[:STEP] -> [LO, LO + STEP .. <= HI]"""
    try:
        parts = [int(v) for v in text.split(':')]
    except ValueError:
        parts = []
    if len(parts) not in (2, 3) or parts[0] < 2 or parts[1] < parts[0] or (len(parts) == 3 and parts[2] < 1):
        raise argparse.ArgumentTypeError("must be LO:HI[:STEP] with 2 <= LO <= HI and STEP >= 1, got %r" % (text,))
    ks = list(range(parts[0], parts[1] + 1, parts[2] if len(parts) == 3 else 1))
    if len(ks) > 64:
        raise argparse.ArgumentTypeError("at most 64 values of k per sweep, got %d" % len(ks))
    return ks


def _eps(text):
    try:
        v = float(text)
    except ValueError:
        v = float('nan')
    if not (v > 0 and v < float('inf')):
        raise argparse.ArgumentTypeError("must be a finite number > 0, got %r" % (text,))
    return v


def _components(text):
    """a count >= 1, or a fraction in (0, 1)"""
    try:
        v = int(text)
    except ValueError:
        try:
            v = float(text)
        except ValueError:
            v = -1.0
        if not 0.0 < v < 1.0:
            raise argparse.ArgumentTypeError("must be an integer >= 1 or a fraction in (0, 1), got %r" % (text,))
        return v
    if v < 1:
        raise argparse.ArgumentTypeError("must be an integer >= 1 or a fraction in (0, 1), got %r" % (text,))
    return v


def _eps_list(text):
    """E1,E2,.. -> [E1, E2 ..]"""
    vals = [_eps(t) for t in text.split(',')]
    if len(vals) > 64:
        raise argparse.ArgumentTypeError("at most 64 values of eps per sweep, got %d" % len(vals))
    return vals


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--inputs', required=True, help=".npy (n, dim) float32 embeddings (eval_embed's output)")
    ap.add_argument('--labels', required=True, help=".npy (n,) strings topic-stance-reason")
    ap.add_argument('--inputs-sp', default=None, help=".npy (n, dim) embeddings of the sampled segmentation: the two *_sp runs")
    ap.add_argument('--posts', default=None, help=".npy (n,) the posts' text, for the CSV's post column (empty without)")
    ap.add_argument('--csv', default=None, help="write the cluster numbers and centroid distances here")
    ap.add_argument('--max-iter', type=int, default=200)
    ap.add_argument('--tsne', default=None, help="write the two-dimensional t-SNE embedding of the inputs here (.npy)")
    ap.add_argument('--tsne-plot', default=None, help="with --tsne: the scatter by topic as an image (needs matplotlib)")
    ap.add_argument('--perplexity', type=float, default=40.0)
    ap.add_argument('--tsne-iter', type=int, default=20000)
    ap.add_argument('--kmeans', type=_positive, default=None, help="also cluster with k-means into this many clusters (VAE.kmeans)")
    ap.add_argument('--kmeans-init', type=_positive, default=10, help="with --kmeans: restarts, the best of which is listed")
    ap.add_argument('--quality', action='store_true', help="a line of silhouette, CH and DB behind every run (VAE.silhouette)")
    ap.add_argument('--sweep', type=_sweep, default=None, help="LO:HI[:STEP]: the k-means quality table for these k per input and metric (VAE.sweep_k)")
    ap.add_argument('--gmm', type=_positive, default=None, help="also fit a Gaussian mixture with this many components (VAE.gmm)")
    ap.add_argument('--gmm-cov', choices=('diag', 'spherical'), default='diag', help="with --gmm / --gmm-sweep: the covariances")
    ap.add_argument('--gmm-init', type=_positive, default=1, help="with --gmm / --gmm-sweep: restarts, the best of which is listed")
    ap.add_argument('--gmm-sweep', type=_sweep, default=None, help="LO:HI[:STEP]: the BIC / AIC table of mixtures for these k per input (VAE.sweep_gmm)")
    ap.add_argument('--dbscan', type=_eps, default=None, help="also cluster by density with this eps (VAE.dbscan)")
    ap.add_argument('--dbscan-min', type=_positive, default=5, help="with --dbscan / --dbscan-sweep: the rows within eps, itself included, that make a row core")
    ap.add_argument('--dbscan-sweep', type=_eps_list, default=None, help="E1,E2,..: the density-clustering quality table for these eps per input and metric (VAE.sweep_eps)")
    ap.add_argument('--pca', type=_components, default=None, help="K or a fraction: first reduce the inputs to their leading principal components (VAE.pca_reduce); every run is made on the reduced rows")
    ap.add_argument('--pca-whiten', action='store_true', help="with --pca: scale the components to unit variance")
    ap.add_argument('--mmd', choices=('stance',), default=None, help="stance: per topic, the kernel two-sample test of its two stances (VAE.mmd, all topics in one call)")
    ap.add_argument('--mmd-perm', type=_positive, default=999, help="with --mmd: the relabelings of the permutation null")
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', type=int, default=0)
    return ap


def main(argv=None):
    from .eval_cluster import make_vae, split_labels
    A = build_parser().parse_args(argv)
    z = np.ascontiguousarray(np.load(A.inputs), dtype=np.float32)
    z_sp = np.ascontiguousarray(np.load(A.inputs_sp), dtype=np.float32) if A.inputs_sp else None
    labels = np.load(A.labels)
    if z.shape[0] != len(labels) or (z_sp is not None and z_sp.shape[0] != len(labels)):
        raise ValueError("one label per row of the inputs")
    if A.tsne_plot and not A.tsne:
        raise ValueError("--tsne-plot needs --tsne")
    vae = make_vae(A.device)
    if A.tsne:
        print(embed(vae, z, labels, A.tsne, A.tsne_plot, A.perplexity, A.tsne_iter, A.seed)[1])
    cols, lines = evaluate(vae, z, z_sp, labels, A.seed, A.max_iter, A.kmeans, A.kmeans_init, A.quality, A.sweep, A.gmm, A.gmm_cov, A.gmm_init,
                           A.gmm_sweep, A.dbscan, A.dbscan_min, A.dbscan_sweep, A.pca, A.pca_whiten, A.mmd, A.mmd_perm)
    for line in lines:
        print(line)
    if A.csv:
        posts = np.load(A.posts) if A.posts else np.array([''] * len(labels))
        write_csv(A.csv, posts, [p[0] for p in split_labels(labels)], [str(v) for v in labels], cols)
    return cols


if __name__ == '__main__':
    main()
