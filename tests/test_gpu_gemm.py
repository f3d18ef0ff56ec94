"""Every GEMM kernel form on its own, through avae_debug_gemm_forced (the caller's tile form and K split reach the kernel as they stand, no
clear is added), against tests/gemm_ref.py: padded leading dimensions, NaN in everything an operand buffer holds beyond the logical operand,
a NaN-payload sentinel in everything of C beyond the logical result, compared through an int32 view.

'exact' cases (integer-valued data, gemm_ref.py) must return the bits of the exact result whatever the kernel family or summation order.
'rounding' cases (wide-range normal draws) are held to gemm_ref.bound().  Largest fraction of the bound seen on MI355X, per family:
    exact-fp32 kernel (gemm_f32.hip), (K_eff + split_k + 3) u magnitude                      0.31 (double-buffered form, K = 32; 0.06-0.19 elsewhere)
    three-way bf16 split (gemm_f32s.hip), 2e-6 (|alpha| |A| |B| + 1)                          0.37 (wave-specialised kernel, K = 1536)
    bf16 operands, conversion passes + gemm_bf16_nt, against products of the rounded operands 0.05
    bf16 operands rounded while staging (bf16_direct), likewise                               0.03
    gemm_tn16 (transposing LDS loads), likewise                                               0.02
    16-bit operands as a producer wrote them, draws rounded to bf16 on the host, same bound:
        gemm_tn16 one slice 0.015, two slices through the slab 0.003 (nine with float atomics 0.001), device-side depth 0.018
        gemm_bf16_pre (A16 the panel itself / transposed from the 2-byte source) 0.034 / 0.002, keep_a16 and the product it feeds 0.017
        K split of the 256x256 NT kernels (phased / register-staged): six slices 0.003 / 0.003, one adding slice 0.046 / 0.046

Which kernel a case reaches.  Exact-fp32 kernel: Case.reach = (tile, fast, db, persist) is what avae_debug_gemm_f32_form -- the function the
launcher itself calls -- returns for the case; tests/test_gemm_ref.py checks that table without a GPU.  The other families, from the
dispatch in the code:
    compute_dtype 2: gemm_split<3> (gemm_f32s.hip): `fast` as in gemm_f32 without the K >= 1536 clause for NT; fast and K per workgroup >= 1536:
        gemm_f32s_ws_kernel (more than 256 tiles: each workgroup walks several), else gemm_f32s_kernel with or without buffer-load staging.
        A pair runs as two launches (gemm_launch).  thin != 0 goes to the exact-fp32 kernel and is not repeated here.
    compute_dtype 1: cvt_bf16 panels, then gemm_bf16_nt: M, N >= 192 and 200 or more 256x256 tiles (gemm_bf16_big_fills): the phased kernel
        (gemm_bf16_p8_ok: K % 64 == 0, K >= 128, N % 4 == 0, ldc % 4 == 0, no device-side K), with option bf16_nt8 = 0 gemm_bf16_nt256_kernel;
        anything smaller: gemm_bf16_nt_kernel (128x128).
    compute_dtype 1, option bf16_direct = 1: gemm_split<1>, dispatch as compute_dtype 2 (the wave-specialised form is off for one plane).
    avae_debug_gemm_tn16: cvt_bf16 row by row, then gemm_bf16_tn: M, N multiples of 8: gemm_bf16_p8_tn, with bf16_nt8 = 0 gemm_bf16_tn256_kernel.
    bf16 mode's 16-bit operands (avae_debug_gemm16: gemm_bf16_pre / gemm_tn16 as the step calls them; the K split of the 256x256 NT kernels through
        avae_debug_gemm_forced; keep_a16 through avae_debug_gemm_call): Case.reach16 = (kernel, slices, slab) is what avae_debug_gemm_bf16_form returns
        -- gemm_bf16_form, the value gemm_bf16_nt / gemm_bf16_tn launch from -- and tests/test_gemm_ref.py holds that table too.  The operand buffers
        are uint16 built on the host: a bf16 NaN in every padding column, guard row and row behind a device-side count; the fp32 pointer of an operand
        given as bf16 is null or all NaN.  Exact cases give the exact bits through the slab, the reduce kernel and float atomics alike; forms without
        float atomics give the bits of the same values converted from fp32 operands.
Not reached by these hooks and left to the existing tests: the fp16 output panel (avae_debug_gemm_c16), the plan's own clears and two-launch
splits (test_gemm_whole_call), and two branches no product of the model reaches: gemm_bf16_nt256_kernel with a device-side depth (a weight gradient
of 200 tiles of 256x256 that gemm_tn16 does not take) and gemm_bf16_p8's clamp to two K tiles per slice (gemm_bf16_slices leaves four)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import gemm_ref as R
from gemm_ref import case

pytestmark = pytest.mark.gpu

L4 = ((0, 0), (0, 1), (1, 1), (1, 0))
KX = (1, 1)
NT = (0, 0)

PRED, FAST, DB_FAST, DB_PRED, PERSIST = (0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 1, 0), (0, 0, 1, 0), (0, 1, 0, 1)
T32, T64, SKINNY = (1, 0, 0, 0), (2, 0, 0, 0), (3, 0, 0, 0)


def _counts(c, counts):
    return [dataclasses.replace(c, count=n, expect=n, name='%s-n%d' % (c.name, n)) for n in counts]


def f32_cases():
    o = []
    # ---- 128x128, predicated staging
    for lay in L4:
        o.append(case('p128', lay, 200, 72, 52, alpha=0.5, bias=True, reach=PRED))
        o.append(case('p128-acc', lay, 333, 260, 132, alpha=-2.0, bias=True, accumulate=1, reach=PRED))
        o.append(case('p128-split3', lay, 333, 260, 132, alpha=0.5, bias=True, split_k=3, reach=PRED))
        o.append(case('p128-split3-acc', lay, 333, 260, 132, split_k=3, accumulate=1, reach=PRED))
        o.append(case('p128-empty-slices', lay, 200, 72, 36, bias=True, split_k=4, reach=PRED))      # 2 K tiles for 4 slices
    o.append(case('p128-rounding', (0, 1), 333, 260, 132, alpha=0.5, bias=True, accumulate=1, data='rounding', reach=PRED))
    o.append(case('p128-rounding-split3', (1, 0), 333, 260, 132, alpha=0.5, bias=True, split_k=3, data='rounding', reach=PRED))
    # ---- 128x128, buffer-load staging
    o.append(case('f128', NT, 333, 256, 1536, alpha=0.5, bias=True, reach=FAST))
    o.append(case('f128', KX, 256, 384, 100, alpha=-2.0, bias=True, accumulate=1, reach=FAST))
    o.append(case('f128-split2', KX, 256, 384, 100, bias=True, split_k=2, reach=FAST))      # kb > 0 enters FastTile::init
    o.append(case('f128', (0, 1), 300, 384, 96, bias=True, reach=FAST))
    o.append(case('f128', (1, 0), 256, 300, 96, bias=True, reach=FAST))
    o.append(case('f128-split2', (0, 1), 300, 384, 96, split_k=2, accumulate=1, reach=FAST))
    o.append(case('f128-rounding-split2', KX, 256, 384, 100, alpha=0.5, bias=True, split_k=2, data='rounding', reach=FAST))
    # ---- 32x128, 64x64, skinny
    for lay in L4:
        for thin, reach in ((1, T32), (2, T64)):
            o.append(case('t%d' % thin, lay, 4, 8, 16, bias=True, thin=thin, reach=reach))
            o.append(case('t%d' % thin, lay, 100, 260, 68, alpha=0.5, bias=True, accumulate=1, thin=thin, reach=reach))
        o.append(case('t2-split2', lay, 100, 260, 68, bias=True, thin=2, split_k=2, reach=T64))
    for lay in (NT, (0, 1)):
        o.append(case('skinny-short-k', lay, 4, 8, 16, bias=True, thin=3, reach=T32))      # K < 64: skinny_ok says no, 32x128 tiles
        o.append(case('skinny', lay, 100, 260, 68, alpha=0.5, bias=True, accumulate=1, thin=3, reach=SKINNY))
        o.append(case('skinny', lay, 96, 200, 64, alpha=-2.0, bias=True, thin=3, reach=SKINNY))
        o.append(case('skinny-short-k', lay, 96, 200, 60, bias=True, thin=3, reach=T32))
    for lay in (KX, (1, 0)):
        o.append(case('skinny-mc', lay, 100, 260, 68, bias=True, thin=3, reach=T32))       # A stored [k][m]: 32x128 tiles
    o.append(case('t1-rounding', NT, 100, 260, 68, alpha=0.5, bias=True, accumulate=1, thin=1, data='rounding', reach=T32))
    o.append(case('t2-rounding', KX, 100, 260, 68, alpha=0.5, bias=True, thin=2, split_k=2, data='rounding', reach=T64))
    o.append(case('skinny-rounding', (0, 1), 100, 260, 68, alpha=0.5, bias=True, accumulate=1, thin=3, data='rounding', reach=SKINNY))
    # ---- double-buffered: 28 x 28 = 784 tiles
    o.append(case('db', (0, 1), 3524, 3584, 32, alpha=0.5, bias=True, reach=DB_FAST))
    o.append(case('db', NT, 3524, 3584, 36, bias=True, accumulate=1, reach=DB_PRED))
    o.append(case('db', KX, 3524, 3584, 32, bias=True, reach=DB_PRED))       # ragged M: predicated
    o.append(case('db-rounding', (0, 1), 3524, 3584, 32, alpha=0.5, bias=True, data='rounding', reach=DB_FAST))
    # ---- persistent: 33 x 32 = 1056 tiles for 768 workgroups, ragged M
    for lay in (NT, (0, 1)):
        o.append(case('persist', lay, 4124, 4096, 64, alpha=0.5, bias=True, accumulate=1, reach=PERSIST))
    o += _counts(case('persist-dyn1', NT, 4124, 4096, 64, bias=True, dyn_kind=1, reach=PERSIST), (4000, 1, 0))
    o.append(case('persist-rounding', NT, 4124, 4096, 64, alpha=0.5, bias=True, accumulate=1, data='rounding', reach=PERSIST))
    o.append(case('persist-from-64x64', NT, 2080, 2048, 32, bias=True, thin=2, reach=PERSIST))     # 33 x 32 tiles of 64x64: the persistent kernel walks 128x128 ones
    # ---- device-side row count
    for lay in L4:
        for thin, split, reach in ((0, 1, PRED), (1, 1, T32), (2, 2, T64)):
            o += _counts(case('dyn1-t%d' % thin, lay, 520, 260, 128, bias=True, thin=thin, split_k=split, dyn_kind=1, reach=reach), (0, 1, 127, 128, 520, 570))
    o += _counts(case('dyn1-fast', KX, 512, 384, 100, bias=True, accumulate=1, dyn_kind=1, reach=FAST), (0, 1, 127, 128, 300))
    # ---- device-side depth, operands [k][x] (the weight gradients); A has a padded leading dimension as the model's 6 D wide arrays
    for thin, reach in ((0, PRED), (1, T32), (2, T64)):
        for split in (1, 3):
            for pair in (False, True):
                o += _counts(case('dyn2-t%d-s%d%s' % (thin, split, '-pair' if pair else ''), KX, 128, 132, 1024, alpha=0.5, bias=split == 1, accumulate=1,
                                  thin=thin, split_k=split, pair=pair, dyn_kind=2, reach=reach), (0, 1, 31, 32, 33, 700, 1074))
    for split in (1, 2):
        o += _counts(case('dyn2-fast-s%d' % split, KX, 128, 256, 1024, accumulate=1, split_k=split, dyn_kind=2, reach=FAST), (0, 1, 31, 32, 33, 700, 1074))
    # ---- pairs: every form that takes one
    for lay in ((0, 1), KX):
        for thin, reach in ((0, PRED), (1, T32), (2, T64), (3, SKINNY if lay == (0, 1) else T32)):
            o.append(case('pair-t%d' % thin, lay, 100, 260, 68, alpha=0.5, bias=True, accumulate=1, thin=thin, pair=True, reach=reach))
    return o


def kcontig_depth_cases(dtype=0):
    """dyn_kind 2 with a k-contiguous operand.  Run as products on the fp32-operand kernels these FAILED on MI355X as the reading of load_tile / s_load
    predicted: with both operands k-contiguous and a count of 5, 6, 7 or 33 every element of C carried the products of the up to three elements
    beyond the count (count 5: 16375 of 16896 elements wrong).  gemm_f32, gemm_f32s and gemm_bf16_direct now refuse the layouts (kernels.h); the
    conversion passes + gemm_bf16_nt mask per element and compute them (bf16_cases)."""
    return [c for lay in (NT, (0, 1), (1, 0))
            for c in _counts(case('dyn2-kcontig', lay, 128, 132, 1024, accumulate=1, dyn_kind=2, dtype=dtype), (5, 6, 7, 33))]


def f32s_cases():
    o = []
    for lay in L4:
        o.append(case('s-plain', lay, 333, 260, 132, alpha=0.5, bias=True, accumulate=1, dtype=2))
        o.append(case('s-plain-split3', lay, 333, 260, 132, bias=True, split_k=3, dtype=2))
    o.append(case('s-fast', KX, 256, 384, 100, alpha=-2.0, bias=True, dtype=2))
    o.append(case('s-fast-split2', KX, 256, 384, 100, bias=True, split_k=2, dtype=2))
    o.append(case('s-ws', NT, 333, 256, 1536, alpha=0.5, bias=True, accumulate=1, dtype=2))
    o.append(case('s-ws-walk', (0, 1), 2100, 2176, 1536, bias=True, dtype=2))        # 17 x 17 = 289 tiles for 256 workgroups
    o += _counts(case('s-ws-dyn1', NT, 333, 256, 1536, bias=True, dyn_kind=1, dtype=2), (0, 130, 400))
    o += _counts(case('s-dyn1', NT, 520, 260, 128, bias=True, dyn_kind=1, dtype=2), (0, 1, 127, 128, 570))
    for split in (1, 3):
        o += _counts(case('s-dyn2-s%d' % split, KX, 128, 132, 1024, accumulate=1, split_k=split, dyn_kind=2, dtype=2), (0, 1, 33, 700, 1074))
    o.append(case('s-pair', (0, 1), 100, 260, 68, alpha=0.5, bias=True, pair=True, dtype=2))
    o.append(case('s-plain-rounding', (0, 1), 333, 260, 132, alpha=0.5, bias=True, accumulate=1, data='rounding', dtype=2))
    o.append(case('s-ws-rounding', NT, 333, 256, 1536, alpha=0.5, bias=True, data='rounding', dtype=2))
    return o


def bf16_cases():
    o = []
    for lay in L4:
        o.append(case('b-nt128', lay, 333, 260, 132, alpha=0.5, bias=True, accumulate=1, dtype=1))
    o.append(case('b-nt128-split3', NT, 333, 260, 132, bias=True, split_k=3, dtype=1))
    o += _counts(case('b-nt128-dyn1', NT, 520, 260, 128, bias=True, dyn_kind=1, dtype=1), (0, 127, 128, 570))
    o += _counts(case('b-nt128-dyn2', KX, 128, 132, 1024, accumulate=1, dyn_kind=2, dtype=1), (0, 33, 700, 1074))
    o += kcontig_depth_cases(1)             # (the panels are k-contiguous whatever the layout: load_panel masks the elements beyond the count)
    o.append(case('b-big', NT, 5000, 2500, 128, alpha=0.5, bias=True, dtype=1))          # 20 x 10 tiles of 256x256
    o += _counts(case('b-big-dyn1', NT, 5000, 2500, 128, bias=True, accumulate=1, dyn_kind=1, dtype=1), (4000,))
    o.append(case('b-nt128-rounding', (0, 1), 333, 260, 132, alpha=0.5, bias=True, accumulate=1, data='rounding', dtype=1))
    o.append(case('b-big-rounding', NT, 5000, 2500, 128, alpha=0.5, bias=True, data='rounding', dtype=1))
    return o


def direct_cases():
    o = [case('d-plain', lay, 333, 260, 132, alpha=0.5, bias=True, accumulate=1, dtype=1) for lay in L4]
    o.append(case('d-fast', KX, 256, 384, 100, alpha=-2.0, bias=True, dtype=1))
    o.append(case('d-fast-split2', KX, 256, 384, 100, bias=True, split_k=2, dtype=1))
    o += _counts(case('d-dyn1', NT, 520, 260, 128, bias=True, dyn_kind=1, dtype=1), (0, 127, 570))
    o += _counts(case('d-dyn2', KX, 128, 132, 1024, accumulate=1, dyn_kind=2, dtype=1), (0, 33, 700, 1074))
    o.append(case('d-rounding', (0, 1), 333, 260, 132, alpha=0.5, bias=True, accumulate=1, data='rounding', dtype=1))
    return o


def tn16_cases():
    """C += alpha A^T B, both operands [k][x]: a Case with accumulate; M, N multiples of 8"""
    return [case('tn16', KX, 136, 264, 100, alpha=0.5, accumulate=1, dtype=1),
            case('tn16', KX, 520, 264, 300, alpha=-2.0, accumulate=1, dtype=1),         # K >= 256: the plan splits K
            case('tn16-rounding', KX, 520, 264, 300, alpha=0.5, accumulate=1, data='rounding', dtype=1)]


# ---------------------------------------------------------------- bf16 mode's 16-bit operand paths
NT128, NT256, P8NT, TN256, P8TN = 0, 1, 2, 3, 4       # GemmBf16Kernel (kernels.h)
SLAB_FLOATS = 512 << 16                                # the slab gemm_tn16 allocates on the handle
DEPTHS = (0, 1, 63, 64, 65, 127, 128, 129, 192, 193, 1000)


def _tn(name, M, N, K, ops, nt8, reach, **kw):
    kw.setdefault('alpha', 0.5)
    return case('%s-%s-nt8=%d' % (name, ops, nt8), KX, M, N, K, accumulate=1, dtype=1, route=1, ops16=ops, nt8=nt8, round16=True, reach16=reach, **kw)


def tn16_producer_cases():
    """one slice: the producers' leading dimensions (A16: the second half of a 2 M wide array; B16: N + 8), each operand as bf16 or as fp32"""
    o = []
    for nt8, kern in ((1, P8TN), (0, TN256)):
        for ops in ('a', 'b', 'ab'):
            o.append(_tn('tn16p', 136, 264, 100, ops, nt8, (kern, 1, 0)))
            o.append(_tn('tn16p', 520, 264, 300, ops, nt8, (kern, 1, 0), alpha=-2.0))       # the plan asks for 2 slices, the launchers run one and ADD
        o.append(_tn('tn16p-rounding', 520, 264, 300, 'ab', nt8, (kern, 1, 0), data='rounding'))
    return o


def tn16_slab_cases():
    """K = 2304: two slices through the slab and p8_slab_reduce_kernel (nt8 = 1), nine with float atomics (nt8 = 0).  264 x 264: four tiles, every one
    an edge tile; 2312 x 264: 10 x 2 tiles -- the second group of tile rows has rows = 2, the last tile row holds 8 rows"""
    o = []
    for M in (264, 2312):
        for nt8, reach in ((1, (P8TN, 2, 1)), (0, (TN256, 9, 0))):
            o.append(_tn('tn16s', M, 264, 2304, 'ab', nt8, reach, alpha=-2.0 if M == 264 else 0.5))
            o.append(_tn('tn16s-rounding', M, 264, 2304, 'ab', nt8, reach, data='rounding'))
    return o


def tn16_depth_cases():
    """a device-side depth, as every weight gradient of a bf16 step passes one.  128 / 129 and 192 / 193: where nkt_all >> 1 changes the DEVICE's slice
    count while the host has launched two slices and the reduce"""
    o = []
    for M, K, nt8, reach in ((264, 2304, 1, (P8TN, 2, 1)), (2312, 2304, 1, (P8TN, 2, 1)), (136, 300, 1, (P8TN, 1, 0)), (264, 2304, 0, (TN256, 9, 0))):
        base = _tn('tn16d', M, 264, K, 'ab', nt8, reach, dyn_kind=2)
        o += _counts(base, tuple(n for n in DEPTHS if n < K) + (K, K + 50))
    o += _counts(_tn('tn16d-rounding', 264, 264, 2304, 'ab', 1, (P8TN, 2, 1), dyn_kind=2, data='rounding'), (193, 1000))
    o += _counts(_tn('tn16d-a', 264, 264, 2304, 'a', 1, (P8TN, 2, 1), dyn_kind=2), (129, 1000))       # B fp32: cvt_bf16 converts its NaN rows too
    return o


def pre_cases():
    """gemm_bf16_pre.  A16 as the k-contiguous panel itself (lda = 2 K: a layer's h out of the two directions' array) against fp32 weights in both
    layouts, and transposed once from the 2-byte source (the dE product where gemm_tn16 does not take the shape: a weight gradient, the K split is
    the plan's).  M = 264: the last 64-column block of transpose_bf16 is partial; K = 100, 1000: its k0 + k < K edge.  All reach the 128x128 kernel;
    gemm_bf16_nt's other branches need 200 tiles of 256x256 (the 256x256 kernel with a device-side depth: 200 such tiles of a weight gradient, which
    no product of the model has) and are covered with converted operands by bf16_cases / nt_split_cases."""
    o = []
    kw = dict(dtype=1, route=0, ops16='a', round16=True, reach16=(NT128, 1, 0))
    for lay in (NT, (0, 1)):
        o.append(case('pre-panel', lay, 333, 264, 136, alpha=0.5, bias=True, **kw))
        o.append(case('pre-panel-acc', lay, 333, 264, 136, alpha=-2.0, bias=True, accumulate=1, **kw))
    o += _counts(case('pre-panel-dyn1', NT, 333, 264, 136, bias=True, dyn_kind=1, **kw), (0, 127, 128, 333))
    o.append(case('pre-panel-rounding', NT, 333, 264, 136, alpha=0.5, bias=True, accumulate=1, data='rounding', **kw))
    for K, slices in ((100, 1), (136, 1), (1000, 7)):
        kw['reach16'] = (NT128, slices, 0)
        o.append(case('pre-transposed', KX, 264, 136, K, alpha=0.5, accumulate=1, wgrad=1, **kw))
    o += _counts(case('pre-transposed-dyn2', KX, 264, 136, 1000, accumulate=1, wgrad=1, dyn_kind=2, **kw), (0, 33, 700, 1000))
    o.append(case('pre-transposed-rounding', KX, 264, 136, 1000, alpha=0.5, accumulate=1, wgrad=1, data='rounding', **kw))
    return o


def nt_split_cases():
    """the K split of the 256x256 NT forms through avae_debug_gemm_forced.  1300 x 1300 x 1536: 36 tiles, the caller's 3 slices re-derived to 6 (216
    items); 5000 x 2500 x 128: 200 tiles, K / 256 = 0 leaves ONE slice, which must add into C as the caller's slices would have.  (gemm_bf16_p8's own
    clamp to two K tiles per slice cannot trigger behind gemm_bf16_slices' four: tests/test_gemm_ref.py sweeps the form for it.)"""
    o = []
    for nt8, kern in ((1, P8NT), (0, NT256)):
        for data in ('exact', 'rounding'):
            kw = dict(dtype=1, nt8=nt8, data=data, round16=True, split_k=3, bias=True, alpha=0.5)
            o.append(case('b-ksplit-%s-nt8=%d' % (data, nt8), NT, 1300, 1300, 1536, reach16=(kern, 6, 0), **kw))
            o.append(case('b-ksplit-one-%s-nt8=%d' % (data, nt8), NT, 5000, 2500, 128, reach16=(kern, 1, 0), **kw))
    return o


def form16(l, c, **over):
    """avae_debug_gemm_bf16_form for a case: [kernel, slices, slab, refused, s2, split asked]"""
    Kp = (c.K + 7) & ~7
    if c.route == 1:
        a = dict(tn=1, wgrad=1, lda=c.lda16 if 'a' in c.ops16 else c.M, ldb=c.ldb16 if 'b' in c.ops16 else c.N, split_k=0)
    elif c.route == 0:
        a = dict(tn=0, wgrad=c.wgrad, lda=Kp if c.a_mc else c.lda16, ldb=Kp, split_k=1)
    else:
        a = dict(tn=0, wgrad=0, lda=Kp, ldb=Kp, split_k=c.split_k)
    a.update(M=c.M, N=c.N, K=c.K, ldc=c.ldc, dyn_kind=c.dyn_kind, bias=int(c.bias), nt8=c.nt8, slab_floats=SLAB_FLOATS)
    a.update(over)
    out = (C.c_int32 * 6)()
    assert l.avae_debug_gemm_bf16_form(a['tn'], a['wgrad'], a['M'], a['N'], a['K'], a['lda'], a['ldb'], a['ldc'], a['split_k'], a['dyn_kind'], a['bias'],
                                       a['nt8'], a['slab_floats'], out) == 0
    return list(out)


def no_atomics(c):
    """does the form the case claims sum in a fixed order?"""
    kern, slices, slab = c.reach16
    return slices == 1 or bool(slab)


F32_CASES = f32_cases()
TN16_CASES = tn16_producer_cases() + tn16_slab_cases() + tn16_depth_cases()
PRE_CASES = pre_cases()
NT_SPLIT_CASES = nt_split_cases()
CASES16 = TN16_CASES + PRE_CASES + NT_SPLIT_CASES
ALL_CASES = F32_CASES + f32s_cases() + bf16_cases() + direct_cases() + tn16_cases() + CASES16
_ids = lambda c: c.id


def env_clean():
    return not [k for k in os.environ if k.startswith('AVAE_F32') or k.startswith('AVAE_BF16D')]


@pytest.fixture(scope='module')
def handles():
    """dtype -> handle, one per compute dtype for the module"""
    from argsim_amd import lib
    assert env_clean(), 'the AVAE_F32* overrides change the dispatch this file pins'
    l = lib.load()
    made = {}

    def get(dtype):
        if dtype not in made:
            cfg = lib.AvaeConfig(32, 16, 8, 1, 1e-4, 1e-3, 2, 1, 0, 0, 1.0, 0.0, dtype)
            h = C.c_void_p()
            assert l.avae_create(C.byref(cfg), 0, C.byref(h)) == 0
            made[dtype] = h
        return made[dtype]

    get.lib = l
    yield get
    for h in made.values():
        l.avae_destroy(h)


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t, shift=0):
    return None if t is None else t.data_ptr() + shift


def launch(get, c, problems, expect=0, shift_a=0, lda=None, K=None, M=None, hook='forced'):
    """-> (return code, error text, the C buffers as they came back)"""
    import torch
    l, h = get.lib, get(c.dtype)
    d = [[_dev(p.A), _dev(p.B), _dev(p.C), _dev(p.bias)] for p in problems]
    cnt = torch.tensor([c.count], dtype=torch.int32).cuda() if c.dyn_kind else None
    two = d[1] if len(d) > 1 else [None] * 4
    M, K, lda = (c.M if M is None else M), (c.K if K is None else K), (c.lda if lda is None else lda)
    if hook == 'tn16':
        rc = l.avae_debug_gemm_tn16(h, _ptr(d[0][0]), _ptr(d[0][1]), _ptr(d[0][2]), M, c.N, K, lda, c.ldb, c.ldc, c.alpha)
    else:
        rc = l.avae_debug_gemm_forced(h, c.a_mc, c.b_nc, _ptr(d[0][0], shift_a), _ptr(d[0][1]), _ptr(d[0][2]), _ptr(d[0][3]), M, c.N, K, lda, c.ldb, c.ldc,
                                      c.alpha, c.accumulate, c.thin, c.split_k, _ptr(cnt), c.dyn_kind, expect, _ptr(two[0]), _ptr(two[1]), _ptr(two[2]), _ptr(two[3]))
    torch.cuda.synchronize()
    return rc, (l.avae_last_error(h) or b'').decode(), [x[2].cpu().numpy() for x in d]


def check(c, problems, got, family):
    want = R.reference(c, problems)
    for i, (p, g, w) in enumerate(zip(problems, got, want)):
        bad = R.untouched(c, g, p.C)
        assert bad.size == 0, (c.id, 'problem %d: written outside the logical result at (row, column)' % i, bad[:5].tolist())
        region = g[:c.M_eff, :c.N]
        if c.data == 'exact':
            ne = np.argwhere(region != w[:c.M_eff, :c.N])
            assert ne.size == 0, (c.id, 'problem %d' % i, len(ne), [(r, k, float(region[r, k]), float(w[r, k])) for r, k in ne[:5].tolist()])
        else:
            ref, bnd = R.bound(c, p, family)
            assert np.isfinite(region).all(), c.id
            frac = float((np.abs(region.astype(np.float64) - ref) / bnd).max()) if ref.size else 0.0
            print('FRAC %s %s %.4f' % (family, c.id, frac))
            assert frac <= 1.0, (c.id, frac)


def run(get, c, family, **kw):
    problems = R.build(c)
    first = None
    for expect in ((0, c.count) if c.dyn_kind == 1 else (0,)):          # the expectation shapes the launch only: never a bit of the result
        rc, err, got = launch(get, c, problems, expect=expect, **kw)
        assert rc == 0, (c.id, err)
        check(c, problems, got, family)
        if first is None:
            first = got
        else:
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(first, got)), (c.id, 'the expected count changed the result')


def refused(get, c, **kw):
    problems = R.build(c)
    rc, err, got = launch(get, c, problems, **kw)
    assert rc != 0 and 'invalid argument' in err, (c.id, rc, err)
    for p, g in zip(problems, got):
        assert np.array_equal(g.view(np.int32), p.C.view(np.int32)), (c.id, 'a refused call wrote to C')


@pytest.mark.parametrize('c', F32_CASES, ids=_ids)
def test_exact_fp32_kernel(handles, c):
    run(handles, c, 'f32')


@pytest.mark.parametrize('family', ['f32', 'f32s', 'direct'])
@pytest.mark.parametrize('c', kcontig_depth_cases(), ids=_ids)
def test_depth_count_needs_kx_operands(handles, c, family):
    """K_eff = min(K, *count) with a k-contiguous operand: the staging tests k < K_eff on the first element of a float4 only, so a count that is no
    multiple of 4 brings in up to three elements beyond it (kcontig_depth_cases).  The launchers refuse the layout; C stays as it was"""
    l, h = handles.lib, handles(1)
    c = dataclasses.replace(c, dtype={'f32': 0, 'f32s': 2, 'direct': 1}[family])
    assert l.avae_set_option(h, b'bf16_direct', int(family == 'direct')) == 0
    try:
        refused(handles, c)
    finally:
        assert l.avae_set_option(h, b'bf16_direct', 0) == 0


@pytest.mark.parametrize('family', ['f32', 'f32s', 'direct', 'bf16'])
def test_depth_count_with_a_k_split_takes_no_bias(handles, family):
    """a slice that starts at or beyond K_eff returns before its epilogue -- slice 0 of a zero depth too, and the bias with it: refused"""
    l, h = handles.lib, handles(1)
    assert l.avae_set_option(h, b'bf16_direct', int(family == 'direct')) == 0
    try:
        for n in (0, 700):
            refused(handles, case('dyn2-split-bias', KX, 128, 132, 1024, bias=True, accumulate=1, split_k=3, dyn_kind=2, count=n,
                                  dtype={'f32': 0, 'f32s': 2}.get(family, 1)))
    finally:
        assert l.avae_set_option(h, b'bf16_direct', 0) == 0


@pytest.mark.parametrize('c', f32s_cases(), ids=_ids)
def test_three_way_split_kernels(handles, c):
    run(handles, c, 'f32s')


@pytest.mark.parametrize('c,nt8', [(c, 1) for c in bf16_cases()] + [(c, 0) for c in bf16_cases() if 'big' in c.name], ids=lambda v: v.id if isinstance(v, R.Case) else 'nt8=%d' % v)
def test_bf16_operand_kernels(handles, c, nt8):
    """nt8 = 1: the phased kernel for the 'b-big' cases; 0: the register-staged 256x256 one.  The 128x128 kernel does not look at the option: run once"""
    l, h = handles.lib, handles(1)
    assert l.avae_set_option(h, b'bf16_nt8', nt8) == 0
    try:
        run(handles, c, 'bf16')
    finally:
        assert l.avae_set_option(h, b'bf16_nt8', 1) == 0


@pytest.mark.parametrize('c', direct_cases(), ids=_ids)
def test_bf16_direct_kernels(handles, c):
    l, h = handles.lib, handles(1)
    assert l.avae_set_option(h, b'bf16_direct', 1) == 0
    try:
        run(handles, c, 'bf16')
    finally:
        assert l.avae_set_option(h, b'bf16_direct', 0) == 0


@pytest.mark.parametrize('nt8', [1, 0])
@pytest.mark.parametrize('c', tn16_cases(), ids=_ids)
def test_gemm_tn16_padded(handles, c, nt8):
    l, h = handles.lib, handles(1)
    assert l.avae_set_option(h, b'bf16_nt8', nt8) == 0
    try:
        run(handles, c, 'bf16', hook='tn16')
    finally:
        assert l.avae_set_option(h, b'bf16_nt8', 1) == 0


@pytest.mark.parametrize('lay', L4)
@pytest.mark.parametrize('what', ['pointer', 'leading dimension', 'contiguous extent'])
def test_refusals(handles, lay, what):
    """a misaligned operand pointer, a leading dimension or a contiguous extent that is no multiple of 4 floats: refused with text, C untouched"""
    c = case('refusal', lay, 200, 72, 52, bias=True, reach=PRED)
    if what == 'pointer':
        refused(handles, c, shift_a=4)
    elif what == 'leading dimension':
        refused(handles, c, lda=c.lda - 2)
    elif lay[0]:
        refused(handles, c, M=c.M - 2)
    else:
        refused(handles, c, K=c.K - 2)


# ---------------------------------------------------------------- bf16 mode's 16-bit operand paths: the tests
def launch16(get, c, p, expect=0, ops=None, **over):
    """one avae_debug_gemm16 call of case c.  ops: which operands go over as bf16 (default: the case's); the fp32 pointer of such an operand is null,
    or with both as bf16 an all-NaN buffer.  -> (return code, error text, C as it came back)"""
    import torch
    l, h = get.lib, get(over.pop('dtype', 1))
    ops = c.ops16 if ops is None else ops
    a16, b16 = R.operands16(dataclasses.replace(c, ops16=ops), p)
    nan = lambda x: np.full_like(x, np.nan) if len(ops) == 2 else None
    dA16, dB16, dC, dbias = _dev(a16), _dev(b16), _dev(p.C), _dev(p.bias)
    dA, dB = _dev(p.A if a16 is None else nan(p.A)), _dev(p.B if b16 is None else nan(p.B))
    cnt = torch.tensor([c.count], dtype=torch.int32).cuda() if c.dyn_kind else None
    a = dict(route=c.route, wgrad=c.wgrad, lda=c.lda if a16 is None else c.lda16, ldb=c.ldb if b16 is None else c.ldb16, dyn_kind=c.dyn_kind, bias=_ptr(dbias))
    a.update(over)
    rc = l.avae_debug_gemm16(h, a['route'], c.a_mc, c.b_nc, a['wgrad'], _ptr(dA16, 2 * c.off16), _ptr(dB16), _ptr(dA), _ptr(dB), _ptr(dC), a['bias'],
                             c.M, c.N, c.K, a['lda'], a['ldb'], c.ldc, c.alpha, c.accumulate, _ptr(cnt), a['dyn_kind'], expect)
    torch.cuda.synchronize()
    return rc, (l.avae_last_error(h) or b'').decode(), dC.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def run16(get, c):
    l, h = get.lib, get(1)
    assert l.avae_set_option(h, b'bf16_nt8', c.nt8) == 0
    try:
        p = R.build(c)[0]
        first = None
        for expect in ((0, c.count) if c.dyn_kind else (0,)):          # the expectation shapes the launch only: never a bit of the result
            rc, err, got = launch16(get, c, p, expect=expect)
            assert rc == 0, (c.id, err)
            check(c, [p], [got], 'bf16')
            if first is None:
                first = got
            else:
                assert _same_bits(first, got), (c.id, 'the expected count changed the result')
        if c.dyn_kind and c.count == 0:
            assert _same_bits(first, p.C), (c.id, 'a count of 0 moved bits of C')
        if c.route == 1 and no_atomics(c):
            # the same values as fp32 operands (cvt_bf16 row by row into dense panels): the same products summed in the same order
            rc, err, got = launch16(get, c, p, ops='')
            assert rc == 0, (c.id, err)
            assert _same_bits(first, got), (c.id, 'bf16 operands as the producer wrote them and the same values converted from fp32 disagree',
                                            np.argwhere(first.view(np.int32) != got.view(np.int32))[:5].tolist())
    finally:
        assert l.avae_set_option(h, b'bf16_nt8', 1) == 0


@pytest.mark.parametrize('c', TN16_CASES, ids=_ids)
def test_gemm_tn16_producer_operands(handles, c):
    """gemm_tn16 with A16 / B16 as the BPTT team kernels and the forward leave them, one slice, through the slab, and under a device-side depth"""
    run16(handles, c)


@pytest.mark.parametrize('c', PRE_CASES, ids=_ids)
def test_gemm_bf16_pre_producer_operand(handles, c):
    run16(handles, c)


@pytest.mark.parametrize('c', NT_SPLIT_CASES, ids=_ids)
def test_bf16_nt_k_split_of_the_big_tiles(handles, c):
    """C holds integers (not zeros) under the caller's split: every slice form, the single re-derived one included, must add onto them"""
    l, h = handles.lib, handles(1)
    problems = R.build(c)
    problems[0].C[:c.M, :c.N] = np.random.default_rng(c.M).integers(-8, 9, (c.M, c.N)).astype(np.float32)
    assert l.avae_set_option(h, b'bf16_nt8', c.nt8) == 0
    try:
        rc, err, got = launch(handles, c, problems)
        assert rc == 0, (c.id, err)
        check(c, problems, got, 'bf16')
    finally:
        assert l.avae_set_option(h, b'bf16_nt8', 1) == 0


def _keep_call(get, A, B, Cbuf, M, N, K, lda, ldb, ldc, a_mc, keep):
    import torch
    l, h = get.lib, get(1)
    dA, dB, dC, dK = _dev(A), _dev(B), _dev(Cbuf), _dev(keep)
    rc = l.avae_debug_gemm_call(h, a_mc, 0, _ptr(dA), _ptr(dB), _ptr(dC), None, M, N, K, lda, ldb, ldc, 1.0, 0, 0, None, 0, None, None, None, _ptr(dK))
    torch.cuda.synchronize()
    assert rc == 0, (l.avae_last_error(h) or b'').decode()
    return dC.cpu().numpy(), dK


def test_keep_a16_is_the_rounded_operand_and_feeds_gemm_tn16(handles):
    """GemmCall::keep_a16: the forward's k-contiguous A operand stays as bf16 [M][K] for the backward's weight gradient.  The panel is bit for bit RNE of
    A, rows beyond M stay as they were; with K % 8 != 0 or A stored [k][m] nothing is kept.  The kept panel is then B16 of a gemm_tn16 product, as
    x16_kept is in the step: dW (136 x 264) += dgi^T x over 300 rows"""
    g = case('keep', KX, 136, 264, 300, alpha=0.5, accumulate=1, dtype=1, route=1, ops16='b', round16=False, data='rounding', reach16=(P8TN, 1, 0))
    p = R.build(g)[0]
    x = p.b.astype(np.float32)                                          # (300, 264): the layer input, NOT yet rounded
    fwd = case('keep-fwd', NT, 300, 72, 264, dtype=1, data='rounding')
    pf = R.build(fwd)[0]
    A = R._operand(x.astype(np.float64), 0)
    keep0 = np.full((300 + R.OP_GUARD_ROWS, 264), R.NAN16, np.uint16)
    got, kept = _keep_call(handles, A, pf.B, pf.C, 300, 72, 264, fwd.lda, fwd.ldb, fwd.ldc, 0, keep0)
    q = dataclasses.replace(pf, a=x.astype(np.float64), A=A)
    check(fwd, [q], [got], 'bf16')
    k = kept.cpu().numpy()
    assert np.array_equal(k[:300], R.bf16_bits(x)) and (k[300:] == R.NAN16).all()
    # handed straight on: the device buffer itself is B16 (ldb = 264)
    import torch
    l, h = handles.lib, handles(1)
    dA, dC = _dev(p.A), _dev(p.C)
    rc = l.avae_debug_gemm16(h, 1, 1, 1, 1, None, _ptr(kept), _ptr(dA), None, _ptr(dC), None, g.M, g.N, g.K, g.lda, 264, g.ldc, g.alpha, 1, None, 0, 0)
    torch.cuda.synchronize()
    assert rc == 0, (l.avae_last_error(h) or b'').decode()
    check(g, [p], [dC.cpu().numpy()], 'bf16')
    # nothing is kept: K % 8 != 0; A stored [k][m]
    for lay, M, K in ((NT, 300, 260), ((1, 0), 300, 264)):
        c = case('keep-not', lay, M, 72, K, dtype=1)
        pc = R.build(c)[0]
        keep0 = np.full((M + R.OP_GUARD_ROWS, (K + 7) & ~7), R.NAN16, np.uint16)
        got, kept = _keep_call(handles, pc.A, pc.B, pc.C, c.M, c.N, c.K, c.lda, c.ldb, c.ldc, c.a_mc, keep0)
        check(c, [pc], [got], 'bf16')
        assert (kept.cpu().numpy() == R.NAN16).all(), (c.id, 'the caller\'s panel was written')


@pytest.mark.parametrize('what', ['rows count', 'bias', 'leading dimension', 'fp32 handle'])
def test_gemm16_refusals(handles, what):
    """refused with text, C's bits untouched"""
    c = _tn('refusal', 136, 264, 100, 'ab', 1, (P8TN, 1, 0))
    p = R.build(dataclasses.replace(c, bias=what == 'bias'))[0]
    if what == 'rows count':
        rc, err, got = launch16(handles, dataclasses.replace(c, dyn_kind=1, count=50), p)
    elif what == 'bias':
        rc, err, got = launch16(handles, c, p)
    elif what == 'leading dimension':
        rc, err, got = launch16(handles, c, p, lda=c.lda16 - 4)
    else:
        rc, err, got = launch16(handles, c, p, dtype=0)
    assert rc != 0 and err, (what, rc, err)
    assert 'invalid argument' in err or what == 'fp32 handle', err
    assert _same_bits(got, p.C), (what, 'a refused call wrote to C')
    if what == 'leading dimension':
        for q in (dataclasses.replace(PRE_CASES[0], bias=False), [x for x in PRE_CASES if x.a_mc][0]):
            pq = R.build(q)[0]
            rc, err, got = launch16(handles, q, pq, lda=q.lda16 - 4)
            assert rc != 0 and 'invalid argument' in err and _same_bits(got, pq.C), (q.id, rc, err)
