"""ctypes boundary to libia.so (include/ia.h).

This is the only way the package reaches the GPU: there is no CPU fallback.  If libia.so is
missing, or no gfx950 device is visible, every entry point raises IAError loudly.
"""
import ctypes
import math
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('IA_LIBIA') or os.path.join(_HERE, 'libia.so')  # override: diagnostic builds

IA_MEM_HOST, IA_MEM_DEVICE = 0, 1
IA_MATCH_F32, IA_MATCH_F16X3 = 0, 1   # option "matcher" (include/ia.h)
_ERRNAMES = {-1: 'IA_EINVAL', -2: 'IA_EHIP', -3: 'IA_ENOMEM', -4: 'IA_ENODEV', -5: 'IA_ECOMM'}


class IAError(RuntimeError):
    pass


class IAShapeError(IAError, ValueError):
    """A list of A images that does not pair up with the A' images (count or shape)."""


class LevelArgs(ctypes.Structure):
    _fields_ = [('ch', ctypes.c_int), ('n_ap', ctypes.c_int), ('a_h', ctypes.c_int), ('a_w', ctypes.c_int),
                ('b_h', ctypes.c_int), ('b_w', ctypes.c_int),
                ('A', ctypes.c_void_p), ('Ac', ctypes.c_void_p), ('Ap', ctypes.c_void_p), ('Apc', ctypes.c_void_p),
                ('B', ctypes.c_void_p), ('Bc', ctypes.c_void_p), ('Bpc', ctypes.c_void_p), ('Bp', ctypes.c_void_p),
                ('weights', ctypes.c_void_p), ('kappa_factor', ctypes.c_double),
                ('s_out', ctypes.c_void_p), ('im_out', ctypes.c_void_p), ('mem', ctypes.c_int),
                ('dbg_src', ctypes.c_void_p), ('dbg_dist', ctypes.c_void_p), ('n_a', ctypes.c_int)]


class Stats(ctypes.Structure):
    _fields_ = [('pixels', ctypes.c_int64), ('steps', ctypes.c_int64), ('coherence_wins', ctypes.c_int64),
                ('reranked', ctypes.c_int64), ('fallbacks', ctypes.c_int64), ('db_ms', ctypes.c_double),
                ('synth_ms', ctypes.c_double), ('dist_launches', ctypes.c_int64), ('dist_flops', ctypes.c_double),
                ('dist_ms', ctypes.c_double), ('dist_launches_timed', ctypes.c_int64),
                ('dist_flops_timed', ctypes.c_double), ('bound_violations', ctypes.c_int64),
                ('f16_levels', ctypes.c_int64), ('pruned_levels', ctypes.c_int64),
                ('dist_pairs', ctypes.c_double), ('dist_pairs_full', ctypes.c_double),
                ('dist_tiles', ctypes.c_double), ('dist_tiles_full', ctypes.c_double),
                ('prune_ms_timed', ctypes.c_double), ('prune_launches_timed', ctypes.c_int64),
                ('prune_flops_timed', ctypes.c_double), ('prune_bytes_timed', ctypes.c_double),
                ('kappa_ambiguous', ctypes.c_int64), ('dist_pairs_corrected', ctypes.c_double),
                ('dist_tiles_rows', ctypes.c_double),
                ('k1b_ms', ctypes.c_double), ('k1b_bytes', ctypes.c_double), ('k1_ms', ctypes.c_double),
                ('k1_bytes', ctypes.c_double), ('build_levels', ctypes.c_int64),
                ('gather_ms_timed', ctypes.c_double), ('gather_launches_timed', ctypes.c_int64),
                ('gather_bytes_timed', ctypes.c_double), ('merge_ms_timed', ctypes.c_double),
                ('merge_launches_timed', ctypes.c_int64), ('build_rows', ctypes.c_int64),
                ('k3p_stamp_ms', ctypes.c_double), ('k3p_stamp_launches', ctypes.c_int64),
                ('k3p_bytes_all', ctypes.c_double), ('merge_stamp_ms', ctypes.c_double),
                ('merge_stamp_launches', ctypes.c_int64), ('stamp_gap_ms', ctypes.c_double),
                ('stamp_gaps', ctypes.c_int64), ('stamp_window_ms', ctypes.c_double), ('prune_rows', ctypes.c_int64),
                ('k3p_stamp_start_ms', ctypes.c_double), ('k3p_stamp_wg_ms', ctypes.c_double),
                ('stamp_gap_sm_ms', ctypes.c_double), ('stamp_gaps_sm', ctypes.c_int64),
                ('k3p_bytes_unique_all', ctypes.c_double),
                ('kcoh_levels', ctypes.c_int64), ('kcoh_fallbacks', ctypes.c_int64), ('kcoh_candidates', ctypes.c_int64),
                ('nbhd_levels', ctypes.c_int64)]

    # fields that describe only the levels with the largest DB seen (build_rows / prune_rows)
    _BUILD = ('k1b_ms', 'k1b_bytes', 'k1_ms', 'k1_bytes', 'build_levels')
    _PRUNE = ('prune_ms_timed', 'prune_launches_timed', 'prune_flops_timed', 'prune_bytes_timed', 'k3p_stamp_ms',
              'k3p_stamp_launches', 'k3p_bytes_all', 'merge_stamp_ms', 'merge_stamp_launches', 'stamp_gap_ms',
              'stamp_gaps', 'stamp_window_ms', 'k3p_stamp_start_ms', 'k3p_stamp_wg_ms', 'stamp_gap_sm_ms',
              'stamp_gaps_sm', 'k3p_bytes_unique_all')

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def add(self, other):
        """accumulate another Stats (e.g. of a concurrent context) field by field (the DB-build
        and pruned-scan timings keep the largest level's, as libia does)"""
        for rows, group in (('build_rows', self._BUILD), ('prune_rows', self._PRUNE)):
            if getattr(other, rows) > getattr(self, rows):
                for k in group:
                    setattr(self, k, 0)
                setattr(self, rows, getattr(other, rows))
        for k, _ in self._fields_:
            if k in ('build_rows', 'prune_rows') or (k in self._BUILD and other.build_rows < self.build_rows) or \
                    (k in self._PRUNE and other.prune_rows < self.prune_rows):
                continue
            setattr(self, k, getattr(self, k) + getattr(other, k))


EXPORTS = {
    'ia_init': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'ia_destroy': (None, [ctypes.c_void_p]),
    'ia_last_error': (ctypes.c_char_p, []),
    'ia_version': (ctypes.c_int, []),
    'ia_set_option': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]),
    'ia_comm_unique_id': (ctypes.c_int, [ctypes.c_char_p]),
    'ia_comm_init': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]),
    'ia_xchg_alloc': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p]),
    'ia_xchg_open': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]),
    'ia_synthesize_levels_kcoh': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(LevelArgs), ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_int, ctypes.POINTER(Stats)]),
    'ia_synthesize_levels_nbhd': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(LevelArgs), ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.POINTER(Stats)]),
    'ia_synthesize_levels_masked': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(LevelArgs), ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                                   ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                   ctypes.POINTER(Stats)]),
    'ia_masked_stats': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]),
    'ia_masked_step_list': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    'ia_pipeline_depend': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'ia_pipeline_generation': (ctypes.c_int, [ctypes.c_void_p]),
    'ia_synthesize_level': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(LevelArgs), ctypes.POINTER(Stats)]),
    'ia_synthesize_levels': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(LevelArgs), ctypes.c_int,
                                            ctypes.POINTER(Stats)]),
    'ia_index_build': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_void_p)]),
    'ia_index_query': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_void_p]),
    'ia_index_query_knn': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_void_p]),
    'ia_index_knn_stats': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'ia_index_similarity': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    'ia_index_count_radius': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    'ia_index_query_radius': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ia_index_set_workspace': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    'ia_index_radius_stats': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'ia_index_destroy': (None, [ctypes.c_void_p]),
    'ia_kmeans': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]),
    'ia_ann_build': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'ia_ann_lists': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'ia_ann_query': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_void_p, ctypes.c_void_p]),
    'ia_ann_stats': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'ia_ann_build_ms': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    'ia_ann_destroy': (None, [ctypes.c_void_p]),
    'ia_coherence_batch': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    'ia_gaussian_pyramid': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'ia_color_matrix': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_int]),
    'ia_k3_microbench': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_double)]),
    'ia_merge_winners': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                        ctypes.c_void_p, ctypes.c_void_p]),
    'ia_chain_budget': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ia_chain_choice': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'ia_wavefront_shape': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int64)]),
    'ia_wavefront_step': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(ctypes.c_int)]),
    'ia_wavefront_shape_pad': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                              ctypes.POINTER(ctypes.c_int64)]),
    'ia_wavefront_step_pad': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                             ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    'ia_shard_tiles': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                      ctypes.POINTER(ctypes.c_int64)]),
    'ia_shard_tiles_pruned': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    'ia_shard_morton_tile': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
}

_lib = None
_lock = threading.Lock()


def lib():
    """Load libia.so (raises IAError if it was not built: run __graft_entry__.build())."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise IAError('libia.so not found at %s — build it with `make -C image-analogies-python_amd/csrc` '
                              'or __graft_entry__.build(); there is no CPU fallback' % LIB_PATH)
            L = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in EXPORTS.items():
                if os.environ.get('IA_LIBIA') and not hasattr(L, name):
                    continue   # a diagnostic / earlier-round library (same-box A/B): its own symbol set
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().ia_last_error()
        raise IAError('%s failed (%s): %s' % (what, _ERRNAMES.get(rc, rc), msg.decode() if msg else ''))


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _c64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def is_pair_list(A):
    """An A side given as a list or tuple holds one image per A' (training pairs (A_i, A'_i));
    a single array is the one A every A' shares (the reference, algorithms.py:63-67)."""
    return isinstance(A, (list, tuple))


def stack_pairs(A_list, Ac_list, n_ap):
    """The A / Ac images of n_ap pairs as the two stacked arrays ia_level_args takes (n_a = n_ap).
    Pairs of different sizes would need a per-image row codec (DB row = img * h * w + r * w + c):
    they are refused, as is a list that has not one A per A'."""
    if not (is_pair_list(A_list) and is_pair_list(Ac_list)):
        raise IAShapeError('A and Ac must both be lists (one image per A\') or both single arrays')
    if len(A_list) != n_ap or len(Ac_list) != n_ap:
        raise IAShapeError("a list of A images needs one A and one Ac per A' image: %d A, %d Ac, %d A'"
                           % (len(A_list), len(Ac_list), n_ap))
    A_list, Ac_list = [_c64(x) for x in A_list], [_c64(x) for x in Ac_list]
    for name, xs in (('A', A_list), ('Ac', Ac_list)):
        if any(x.shape != xs[0].shape for x in xs):
            raise IAShapeError('every %s of a pair list must have one shape (got %s); pairs of different sizes '
                               'are not supported' % (name, [x.shape for x in xs]))
    return _c64(np.stack(A_list)), _c64(np.stack(Ac_list))


NBHD_N_SM, NBHD_N_LG, NBHD_MAX_D = (1, 3, 5), (3, 5, 7, 9), 167   # ia_synthesize_levels_nbhd's sizes (include/ia.h)


def feature_width(n_sm, n_lg, ch):
    """D of a DB row with n_sm x n_sm coarse and n_lg x n_lg fine windows: ch (2 n_sm^2 + n_lg^2 + n_lg^2 // 2)"""
    return ch * (2 * n_sm * n_sm + n_lg * n_lg + (n_lg * n_lg) // 2)


def check_level_shapes(A, Ac, Ap, Apc, B, Bc, Bpc, Bp, w, windows=(3, 5)):
    """The C ABI derives every size from A's channel count and B's shape (include/ia.h
    ia_level_args); check the rest here so a mismatched call raises instead of reading or
    writing past a host buffer.  Ap / Apc are the stacked A' images.  windows: the level's
    (n_sm, n_lg), which set the weights' length.  Returns ch."""
    if A.ndim not in (2, 3):
        raise IAError('A must be (h, w) or (h, w, ch)')
    ch = 1 if A.ndim == 2 else A.shape[2]
    if not 1 <= ch <= 3:
        raise IAError('images must have 1, 2 or 3 channels (got %d)' % ch)
    half = lambda x: (-(-x.shape[0] // 2), -(-x.shape[1] // 2)) + x.shape[2:]
    if B.ndim != A.ndim or B.shape[2:] != A.shape[2:]:
        raise IAError('B must have the channel count of A: %s vs %s' % (B.shape, A.shape))
    if Ap.ndim != A.ndim + 1 or Ap.shape[1:] != A.shape or Ap.shape[0] < 1:
        raise IAError("every A' level must have A's shape %s (got %s)" % (A.shape, Ap.shape[1:]))
    if Ac.shape != half(A):
        raise IAError('Ac must be the coarser level of A, %s (got %s)' % (half(A), Ac.shape))
    if Apc.shape != (Ap.shape[0],) + half(A):
        raise IAError("every coarse A' level must be %s (got %s)" % (half(A), Apc.shape[1:]))
    for name, x in (('Bc', Bc), ('Bpc', Bpc)):
        if x.shape != half(B):
            raise IAError('%s must be the coarser level of B, %s (got %s)' % (name, half(B), x.shape))
    if Bp.shape != B.shape:
        raise IAError("Bp must have B's shape %s (got %s)" % (B.shape, Bp.shape))
    if tuple(windows) == (3, 5):
        if w.shape != (55 * ch,):
            raise IAError('weights must have 55 * ch = %d entries (3x3 / 5x5 windows; got %s)' % (55 * ch, w.shape))
    elif w.shape != (feature_width(windows[0], windows[1], ch),):
        raise IAError('weights must have %d entries (%dx%d / %dx%d windows, %d channels; got %s)'
                      % (feature_width(windows[0], windows[1], ch), windows[0], windows[0], windows[1], windows[1], ch,
                         w.shape))
    return ch


def check_mask_state(B, mask, s, im):
    """The mask and the kept state of a masked level call, as the C ABI reads them (include/ia.h
    ia_synthesize_levels_masked): mask (b_h, b_w) bool or uint8, s (N, 2) and im (N,) integers, N = b_h b_w;
    s = im = None: no kept pixel has a source (im = -1).  A mismatch raises instead of reading past a buffer.
    Returns (mask uint8, s int32 (N, 2), im int32 (N,)), each a fresh C-contiguous array."""
    bh, bw = B.shape[:2]
    n = bh * bw
    mask = np.asarray(mask)
    if mask.shape != (bh, bw) or mask.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        raise IAError('mask must be a bool or uint8 array of B\'s shape %s (got %s %s)' % ((bh, bw), mask.dtype, mask.shape))
    if (s is None) != (im is None):
        raise IAError('s and im are given together or not at all')
    if s is None:
        return np.array(mask, dtype=np.uint8, order='C'), np.zeros((n, 2), dtype=np.int32), np.full(n, -1, dtype=np.int32)
    s, im = np.asarray(s), np.asarray(im)
    if s.shape != (n, 2) or im.shape != (n,) or s.dtype.kind != 'i' or im.dtype.kind != 'i':
        raise IAError('s must be (%d, 2) and im (%d,) integer arrays (got %s %s, %s %s)'
                      % (n, n, s.dtype, s.shape, im.dtype, im.shape))
    return np.array(mask, dtype=np.uint8, order='C'), np.array(s, dtype=np.int32, order='C'), np.array(im, dtype=np.int32, order='C')


def _a_side(A, Ac, Ap_list, Apc_list):
    """The A side of a host level call: (A, Ac, A_all, Ac_all, Ap, Apc, n_a).  A / Ac: one image, what the
    shapes are checked on; A_all / Ac_all: what the library reads, (n_a, h, w[, ch]) when A or Ac is a list
    with one image per A' (pairs; n_a = n_ap), else the one shared image (n_a = 0)."""
    Ap = _c64(np.stack(Ap_list))
    Apc = _c64(np.stack(Apc_list))
    if is_pair_list(A) or is_pair_list(Ac):
        A_all, Ac_all = stack_pairs(A, Ac, Ap.shape[0])
        return A_all[0], Ac_all[0], A_all, Ac_all, Ap, Apc, Ap.shape[0]
    A, Ac = _c64(A), _c64(Ac)
    return A, Ac, A, Ac, Ap, Apc, 0


def _host_job(a_side, jb, windows, masked):
    """One job of a host level call: its arrays converted and checked against the A side, its maps s / im
    (masked: the checked copies of the job's kept state, which the call updates; else fresh ones), its debug
    records (a job with a debug dict, not masked) and its LevelArgs.  Returns (LevelArgs, the converted
    arrays - the mask last - which the caller keeps alive through the call, s, im, dsrc, ddist)."""
    A, Ac, A_all, Ac_all, Ap, Apc, n_a = a_side
    B, Bc, Bpc, Bp, w = _c64(jb['B']), _c64(jb['Bc']), _c64(jb['Bpc']), jb['Bp'], _c64(jb['weights'])
    if not (isinstance(Bp, np.ndarray) and Bp.dtype == np.float64 and Bp.flags.c_contiguous):
        raise IAError('Bp must be a C-contiguous float64 array (updated in place)')
    ch = check_level_shapes(A, Ac, Ap, Apc, B, Bc, Bpc, Bp, w, windows=windows)
    bh, bw = B.shape[:2]
    kept, dsrc, ddist = (B, Bc, Bpc, w), None, None
    if masked:
        mask, s, im = check_mask_state(B, jb['mask'], jb.get('s'), jb.get('im'))   # s / im: in and out (they may alias)
        kept += (mask,)
    else:
        s, im = np.empty((bh * bw, 2), dtype=np.int32), np.empty(bh * bw, dtype=np.int32)
        if jb.get('debug') is not None:
            dsrc = np.zeros((bh * bw, 6), dtype=np.int32)
            ddist = np.zeros((bh * bw, 2), dtype=np.float64)
    args = LevelArgs(ch, Ap.shape[0], A.shape[0], A.shape[1], bh, bw,
                     _ptr(A_all), _ptr(Ac_all), _ptr(Ap), _ptr(Apc), _ptr(B), _ptr(Bc), _ptr(Bpc), _ptr(Bp),
                     _ptr(w), float(jb['kappa_factor']), _ptr(s), _ptr(im), IA_MEM_HOST,
                     None if dsrc is None else _ptr(dsrc), None if ddist is None else _ptr(ddist), n_a)
    return args, kept, s, im, dsrc, ddist


def _device_jobs(ch, n_ap, a_hw, b_hw, ptr_list, kappa_factors, n_a):
    """The LevelArgs array of a device level call: one ptrs dict and kappa factor per job; n_a: one value for
    all jobs or one per job."""
    args = []
    n_as = list(n_a) if isinstance(n_a, (list, tuple)) else [n_a] * len(ptr_list)
    for ptrs, kf, na in zip(ptr_list, kappa_factors, n_as):
        p = {k: ctypes.c_void_p(int(v)) for k, v in ptrs.items()}
        args.append(LevelArgs(ch, n_ap, a_hw[0], a_hw[1], b_hw[0], b_hw[1], p['A'], p['Ac'], p['Ap'], p['Apc'],
                              p['B'], p['Bc'], p['Bpc'], p['Bp'], p['weights'], float(kf),
                              p['s_out'], p['im_out'], IA_MEM_DEVICE, None, None, int(na)))
    return (LevelArgs * len(args))(*args)


class Context(object):
    """One GPU (ia_ctx).  device: HIP ordinal (default: LOCAL_RANK or 0)."""

    def __init__(self, device=None):
        if device is None:
            device = int(os.environ.get('LOCAL_RANK', 0))
        self._h = ctypes.c_void_p()
        self._opts = {}
        check(lib().ia_init(device, ctypes.byref(self._h)), 'ia_init(%d)' % device)
        self.device = device

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().ia_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        check(lib().ia_set_option(self._h, name.encode(), int(value)), 'ia_set_option')
        self._opts[name] = int(value)

    def option(self, name, default=None):
        """The value last set for option `name` on this context (the C ABI has no getter), or
        `default` - the caller's statement of the library default - when it was never set."""
        return self._opts.get(name, default)

    def gaussian_pyramid(self, img, n_reduce, weights7):
        """ia_gaussian_pyramid on a host array: the n_reduce successive pyramid_reduce levels of
        img (finest first), as a list of arrays."""
        img = _c64(img)
        h, w = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        shapes, hh, ww = [], h, w
        for _ in range(n_reduce):
            hh, ww = (hh + 1) // 2, (ww + 1) // 2
            shapes.append((hh, ww) + img.shape[2:])
        out = np.empty(sum(int(np.prod(x)) for x in shapes) or 1, dtype=np.float64)
        w7 = _c64(weights7)
        check(lib().ia_gaussian_pyramid(self._h, _ptr(img), h, w, ch, n_reduce, _ptr(w7), _ptr(out), IA_MEM_HOST),
              'ia_gaussian_pyramid')
        res, off = [], 0
        for shp in shapes:
            n = int(np.prod(shp))
            res.append(out[off:off + n].reshape(shp))
            off += n
        return res

    def color_matrix(self, img, M):
        """ia_color_matrix: np.einsum('ij,klj->kli', M, img) for an (h, w, 3) host array."""
        img = _c64(img)
        if img.ndim != 3 or img.shape[2] != 3:
            raise IAError('color_matrix: (h, w, 3) image expected')
        out = np.empty_like(img)
        M = _c64(M)
        check(lib().ia_color_matrix(self._h, _ptr(img), img.shape[0] * img.shape[1], _ptr(M), _ptr(out), IA_MEM_HOST),
              'ia_color_matrix')
        return out

    def k3_microbench(self, n_rows, M, reps=20):
        """Mean device microseconds of one split-f16 distance-scan launch (random operands)."""
        us = ctypes.c_double()
        check(lib().ia_k3_microbench(self._h, int(n_rows), int(M), int(reps), ctypes.byref(us)), 'ia_k3_microbench')
        return us.value

    def comm_init(self, rank, world, uid):
        check(lib().ia_comm_init(self._h, rank, world, bytes(uid)), 'ia_comm_init')

    def xchg_init(self, rank, world, all_gather):
        """Peer-write winner exchange of sharded levels (include/ia.h ia_xchg_alloc/open):
        all_gather(bytes) -> list of every rank's bytes in rank order (e.g. a torch.distributed
        all_gather_object wrapper).  Makes this context rank `rank` of a world-rank DB shard."""
        h = ctypes.create_string_buffer(64)
        rc = lib().ia_xchg_alloc(self._h, world, h)
        hs = all_gather(h.raw if rc == 0 else b'')   # every rank takes part, even after a failure
        check(rc, 'ia_xchg_alloc')
        if len(hs) != world or any(len(x) != 64 for x in hs):
            raise IAError('xchg_init: expected %d handles of 64 bytes (a peer failed ia_xchg_alloc)' % world)
        check(lib().ia_xchg_open(self._h, rank, world, b''.join(hs)), 'ia_xchg_open')

    def pipeline_depend(self, prev, gen):
        """The next level call on this context waits, step by step, for the level call number
        `gen` of `prev` (a context with option pipeline_record = 1) - include/ia.h."""
        check(lib().ia_pipeline_depend(self._h, prev.handle if prev is not None else None, int(gen)),
              'ia_pipeline_depend')

    def pipeline_generation(self):
        return lib().ia_pipeline_generation(self._h)

    def synthesize_level(self, A, Ac, Ap_list, Apc_list, B, Bc, Bpc, Bp, weights, kappa_factor, stats=None,
                         debug=None, sim=None, windows=None):
        """ia_synthesize_level on host numpy arrays.  A / Ac: one array each (the A every A' shares)
        or lists with one array per A' (pairs (A_i, A'_i) of equal shape; IAShapeError, a
        ValueError, otherwise).  Bp (fp64, C-contiguous) is updated in place
        (the reference mutates Bp_pyr[level], image_analogies.py:214).  Returns (s, im):
        s (N, 2) int32 source pixel in A', im (N,) int32 source A' image, raster order.
        debug: a dict to receive the debug=True per-pixel records (include/ia.h dbg_src/dbg_dist):
        'src' (N, 6) int32 [p_app row, col, img, r_star row, col, has_coh], 'dist' (N, 2) fp64
        [d_app, d_coh] (image_analogies.py:224-240), finished on the host as numpy does.
        sim: (N_A, K) similarity sets of the level's DB rows (ExactIndex.similarity): the level runs
        by k-coherence search (include/ia.h ia_synthesize_levels_kcoh) - not the reference's result unless
        K = N_A - 1; None: the exact path.
        windows: (n_sm, n_lg): the level runs through ia_synthesize_levels_nbhd with those window sizes
        (weights then hold feature_width(n_sm, n_lg, ch) values; no debug, no sim); None: the default
        call, 3 / 5."""
        job = dict(B=B, Bc=Bc, Bpc=Bpc, Bp=Bp, weights=weights, kappa_factor=kappa_factor, debug=debug)
        return self.synthesize_levels(A, Ac, Ap_list, Apc_list, [job], stats, sim=sim, windows=windows)[0]

    def synthesize_levels(self, A, Ac, Ap_list, Apc_list, jobs, stats=None, sim=None, windows=None):
        """ia_synthesize_levels: one level of several jobs that share the A side (A, A' levels l and
        l-1), e.g. a kappa / pyramid-depth sweep (multi_script.py).  jobs: list of dicts with
        B, Bc, Bpc, Bp (updated in place), weights, kappa_factor and optionally debug (a dict, see
        synthesize_level).  A / Ac may be lists, one image per A' (pairs), as in synthesize_level.
        One DB, one distance scan per wavefront step for all jobs.  Returns
        [(s, im)] per job, each identical to a separate synthesize_level call.
        sim: the A side's similarity sets, shared by every job (synthesize_level).
        windows: (n_sm, n_lg) for every job, or None (synthesize_level)."""
        if windows is not None:
            windows = (int(windows[0]), int(windows[1]))
            if sim is not None or any(jb.get('debug') is not None for jb in jobs):
                raise IAError('synthesize_levels: windows= takes neither sim nor debug (ia_synthesize_levels_nbhd)')
        if not 1 <= len(jobs) <= 32:
            raise IAError('synthesize_levels: 1..32 jobs per call (got %d)' % len(jobs))
        a_side = _a_side(A, Ac, Ap_list, Apc_list)
        A, Ap = a_side[0], a_side[4]
        sim_k = 0
        if sim is not None:
            sim = np.ascontiguousarray(sim, dtype=np.int32)
            if sim.ndim != 2 or sim.shape[0] != Ap.shape[0] * A.shape[0] * A.shape[1]:
                raise IAError('sim must be (N_A, K) = (%d, K) (got %s)' % (Ap.shape[0] * A.shape[0] * A.shape[1], sim.shape))
            sim_k = sim.shape[1]
        keep, args, outs = [], [], []
        for jb in jobs:
            a, kept, s, im, dsrc, ddist = _host_job(a_side, jb, windows or (3, 5), False)
            args.append(a)
            keep.append(kept)
            outs.append((s, im, dsrc, ddist, jb.get('debug')))
        arr = (LevelArgs * len(args))(*args)
        st = stats if stats is not None else Stats()
        if windows is not None:
            check(lib().ia_synthesize_levels_nbhd(self._h, arr, len(args), windows[0], windows[1], ctypes.byref(st)),
                  'ia_synthesize_levels_nbhd')
        elif sim is None:
            check(lib().ia_synthesize_levels(self._h, arr, len(args), ctypes.byref(st)), 'ia_synthesize_levels')
        else:
            check(lib().ia_synthesize_levels_kcoh(self._h, arr, len(args), _ptr(sim), sim_k, ctypes.byref(st)),
                  'ia_synthesize_levels_kcoh')
        res = []
        for s, im, dsrc, ddist, debug in outs:
            if debug is not None:
                # compute_distance = norm(x) ** 2 on numpy scalars: sqrt, then libm pow(., 2), which
                # can differ from sqrt(v) * sqrt(v) by 1 ulp; finish it here exactly like that
                for qi in np.flatnonzero(dsrc[:, 5]):
                    ddist[qi, 0] = math.sqrt(ddist[qi, 0]) ** 2
                    ddist[qi, 1] = math.sqrt(ddist[qi, 1]) ** 2
                debug['src'], debug['dist'] = dsrc, ddist
            res.append((s, im))
        return res

    def synthesize_level_device(self, ch, n_ap, a_hw, b_hw, ptrs, kappa_factor, stats=None, n_a=0, sim=None, sim_k=0,
                                windows=None):
        """Same on device pointers (IA_MEM_DEVICE): ptrs = dict of int addresses for
        A, Ac, Ap, Apc, B, Bc, Bpc, Bp, weights, s_out, im_out (e.g. torch tensor data_ptr()).
        n_a = n_ap: A and Ac stack one image per A' (pairs); 0 or 1: one shared A.
        sim_k = K > 0: sim is the device address of the (N_A, K) int32 similarity sets (k-coherence search).
        windows = (n_sm, n_lg): ia_synthesize_levels_nbhd (the weights hold feature_width(n_sm, n_lg, ch) values)."""
        return self.synthesize_levels_device(ch, n_ap, a_hw, b_hw, [ptrs], [kappa_factor], stats, n_a=n_a, sim=sim,
                                             sim_k=sim_k, windows=windows)

    def synthesize_levels_device(self, ch, n_ap, a_hw, b_hw, ptr_list, kappa_factors, stats=None, n_a=0, sim=None, sim_k=0,
                                 windows=None):
        """ia_synthesize_levels on device pointers: one ptrs dict per job (the A-side addresses
        must be equal in all of them), one kappa factor per job; n_a as in synthesize_level_device,
        or a list with one value per job (the library refuses jobs that differ).  sim / sim_k: the A side's
        similarity sets on the device, for every job (synthesize_level_device)."""
        arr = _device_jobs(ch, n_ap, a_hw, b_hw, ptr_list, kappa_factors, n_a)
        st = stats if stats is not None else Stats()
        if windows is not None:
            if sim is not None or sim_k:
                raise IAError('synthesize_levels_device: windows= takes no sim (ia_synthesize_levels_nbhd)')
            check(lib().ia_synthesize_levels_nbhd(self._h, arr, len(arr), int(windows[0]), int(windows[1]), ctypes.byref(st)),
                  'ia_synthesize_levels_nbhd')
        elif sim is None and not sim_k:
            check(lib().ia_synthesize_levels(self._h, arr, len(arr), ctypes.byref(st)), 'ia_synthesize_levels')
        else:
            check(lib().ia_synthesize_levels_kcoh(self._h, arr, len(arr), None if sim is None else ctypes.c_void_p(int(sim)),
                                                  int(sim_k), ctypes.byref(st)), 'ia_synthesize_levels_kcoh')
        return st

    def resynthesize_levels(self, A, Ac, Ap_list, Apc_list, jobs, windows=(3, 5), stats=None):
        """ia_synthesize_levels_masked on host arrays: redo the masked pixels of one level
        of several jobs that share the A side, and keep the rest exactly.  jobs: dicts as in synthesize_levels
        (B, Bc, Bpc, Bp, weights, kappa_factor) plus mask (bool or uint8, b_h x b_w: True = redo) and s, im:
        the previous state ((N, 2) and (N,); im < 0 = a kept pixel without a source; both None = none has
        one).  Bp holds the kept values and is updated in place at the masked pixels only.  windows: (n_sm,
        n_lg) for every job.  Returns [(s, im)]: the complete new maps (fresh arrays; the inputs are not
        written)."""
        windows = (int(windows[0]), int(windows[1]))
        if not 1 <= len(jobs) <= 32:
            raise IAError('resynthesize_levels: 1..32 jobs per call (got %d)' % len(jobs))
        a_side = _a_side(A, Ac, Ap_list, Apc_list)
        keep, args, outs = [], [], []
        for jb in jobs:
            a, kept, s, im, _, _ = _host_job(a_side, jb, windows, True)
            args.append(a)
            keep.append(kept)
            outs.append((s, im))
        n = len(args)
        arr = (LevelArgs * n)(*args)
        pm = (ctypes.c_void_p * n)(*[k[4].ctypes.data for k in keep])
        ps = (ctypes.c_void_p * n)(*[o[0].ctypes.data for o in outs])
        pi = (ctypes.c_void_p * n)(*[o[1].ctypes.data for o in outs])
        st = stats if stats is not None else Stats()
        check(lib().ia_synthesize_levels_masked(self._h, arr, n, windows[0], windows[1], pm, ps, pi, ctypes.byref(st)),
              'ia_synthesize_levels_masked')
        return outs

    def resynthesize_levels_device(self, ch, n_ap, a_hw, b_hw, ptr_list, kappa_factors, windows=(3, 5), stats=None, n_a=0):
        """ia_synthesize_levels_masked on device pointers: one ptrs dict per job as in synthesize_levels_device,
        plus 'mask' (N bytes), 's_in' (N x 2 int32) and 'im_in' (N int32) addresses; s_in / im_in may equal
        s_out / im_out."""
        arr = _device_jobs(ch, n_ap, a_hw, b_hw, ptr_list, kappa_factors, n_a)
        n = len(arr)
        pm, ps, pi = ((ctypes.c_void_p * n)(*[int(p[k]) for p in ptr_list]) for k in ('mask', 's_in', 'im_in'))
        st = stats if stats is not None else Stats()
        check(lib().ia_synthesize_levels_masked(self._h, arr, n, int(windows[0]), int(windows[1]), pm, ps, pi,
                                                ctypes.byref(st)), 'ia_synthesize_levels_masked')
        return st

    def masked_stats(self):
        """ia_masked_stats: (levels (jobs) this context's masked calls ran, device ms of their step lists)"""
        n, ms = ctypes.c_int64(), ctypes.c_double()
        check(lib().ia_masked_stats(self._h, ctypes.byref(n), ctypes.byref(ms)), 'ia_masked_stats')
        return n.value, ms.value


KNN_MAX = 64  # IA_KNN_MAX of include/ia.h
KCOH_MAX = 15  # IA_KCOH_MAX


class ExactIndex(object):
    """ia_index_*: exact 1-NN, k-NN and fixed-radius search over fp64 rows (FLANN `linear` semantics, numpy
    summation order)."""

    def __init__(self, ctx, pts):
        pts = _c64(pts)
        if pts.ndim != 2 or pts.shape[0] < 1:
            raise IAError('ExactIndex: pts must be a non-empty (n, d) array')
        self.ctx = ctx
        self.n, self.d = pts.shape
        self._h = ctypes.c_void_p()
        check(lib().ia_index_build(ctx.handle, _ptr(pts), self.n, self.d, ctypes.byref(self._h)), 'ia_index_build')

    def query(self, q):
        q = _c64(np.atleast_2d(q))
        if q.shape[1] != self.d:
            raise IAError('ExactIndex.query: query width %d != index width %d' % (q.shape[1], self.d))
        idx = np.empty(q.shape[0], dtype=np.int64)
        dist = np.empty(q.shape[0], dtype=np.float64)
        check(lib().ia_index_query(self._h, _ptr(q), q.shape[0], _ptr(idx), _ptr(dist)), 'ia_index_query')
        return idx, dist

    def query_knn(self, q, k):
        """ia_index_query_knn: the k nearest rows of every query, ascending (distance, index), lowest
        index on ties; 1 <= k <= min(n, KNN_MAX).  Returns (idx (nq, k) int64, dist (nq, k) float64)."""
        q = _c64(np.atleast_2d(q))
        if q.shape[1] != self.d:
            raise IAError('ExactIndex.query_knn: query width %d != index width %d' % (q.shape[1], self.d))
        k = int(k)
        idx = np.empty((q.shape[0], max(k, 0)), dtype=np.int64)
        dist = np.empty((q.shape[0], max(k, 0)), dtype=np.float64)
        check(lib().ia_index_query_knn(self._h, _ptr(q), q.shape[0], k, _ptr(idx), _ptr(dist)), 'ia_index_query_knn')
        return idx, dist

    def similarity(self, K):
        """ia_index_similarity: (n, K) int32, row j = the K rows most similar to row j under query_knn's
        order, j itself left out (the similarity sets of k-coherence search); 1 <= K <= min(KCOH_MAX, n - 1)."""
        K = int(K)
        sim = np.empty((self.n, max(K, 0)), dtype=np.int32)
        check(lib().ia_index_similarity(self._h, K, _ptr(sim)), 'ia_index_similarity')
        return sim

    def knn_stats(self):
        """ia_index_knn_stats of the last query_knn: (rows whose exact fp64 distance was computed,
        scan chunks rescanned exactly)."""
        out = (ctypes.c_int64 * 2)()
        check(lib().ia_index_knn_stats(self._h, out), 'ia_index_knn_stats')
        return int(out[0]), int(out[1])

    def _radius_args(self, what, q, radius):
        q = _c64(np.atleast_2d(q))
        if q.shape[1] != self.d:
            raise IAError('ExactIndex.%s: query width %d != index width %d' % (what, q.shape[1], self.d))
        r = np.asarray(radius, dtype=np.float64)
        if r.ndim == 0:
            r = np.full(q.shape[0], float(r))
        r = np.ascontiguousarray(r)
        if r.shape != (q.shape[0],):
            raise IAError('ExactIndex.%s: radius must be a scalar or one value per query' % what)
        return q, r

    def count_radius(self, q, radius):
        """ia_index_count_radius: per query the exact number of rows with squared distance < radius
        (a scalar or one value per query), int64 (nq,)."""
        q, r = self._radius_args('count_radius', q, radius)
        count = np.empty(q.shape[0], dtype=np.int64)
        check(lib().ia_index_count_radius(self._h, _ptr(q), q.shape[0], _ptr(r), _ptr(count)), 'ia_index_count_radius')
        return count

    def query_radius(self, q, radius, max_nn=None):
        """ia_index_query_radius: the rows with squared distance < radius, nearest first, ties to the
        lower index.  max_nn = None: the exact CSR form (offsets (nq + 1,), idx, dist), query j's rows at
        offsets[j]:offsets[j + 1] (a counting call, then the query).  max_nn = m >= 1: (idx (nq, m),
        dist (nq, m), count (nq,)) with the m nearest, padded with -1 / +inf; count is the full count."""
        q, r = self._radius_args('query_radius', q, radius)
        nq = q.shape[0]
        if max_nn is None:
            offsets = np.zeros(nq + 1, dtype=np.int64)
            np.cumsum(self.count_radius(q, r), out=offsets[1:])
        else:
            if int(max_nn) < 1:
                raise IAError('ExactIndex.query_radius: max_nn must be None or >= 1 (got %r)' % (max_nn,))
            offsets = np.arange(nq + 1, dtype=np.int64) * int(max_nn)
        idx = np.empty(int(offsets[-1]), dtype=np.int64)
        dist = np.empty(int(offsets[-1]), dtype=np.float64)
        count = np.empty(nq, dtype=np.int64)
        check(lib().ia_index_query_radius(self._h, _ptr(q), nq, _ptr(r), _ptr(offsets), _ptr(idx), _ptr(dist),
                                          _ptr(count)), 'ia_index_query_radius')
        if max_nn is None:
            return offsets, idx, dist
        return idx.reshape(nq, int(max_nn)), dist.reshape(nq, int(max_nn)), count

    def set_workspace(self, entries):
        """ia_index_set_workspace: candidate entries a radius call keeps on the device per fill pass
        (0: the default)."""
        check(lib().ia_index_set_workspace(self._h, int(entries)), 'ia_index_set_workspace')

    def radius_stats(self):
        """ia_index_radius_stats of the last radius call: ((query, row) pairs verified in fp64, rows found
        inside, fill sub-batches, query segments sorted outside LDS)."""
        out = (ctypes.c_int64 * 4)()
        check(lib().ia_index_radius_stats(self._h, out), 'ia_index_radius_stats')
        return tuple(int(v) for v in out)

    def coherence(self, q, px, s, im, A_hw, Bp_w, pad=2):
        """ia_coherence_batch: best_coherence_match (algorithms.py:92-130) of every pixel px[i]
        (row, col) with query feature q[i], against this index's rows (As).  s (n, 2) / im (n)
        must cover every causal neighbour of the batch.  Returns (p (nq, 2), img (nq,),
        r_star (nq, 2)) as int32; p = (-1, -1), img 0, r_star (0, 0) where there is no candidate."""
        q = _c64(np.atleast_2d(q))
        px = np.ascontiguousarray(np.atleast_2d(px), dtype=np.int32)
        s = np.ascontiguousarray(np.asarray(s).reshape(-1, 2), dtype=np.int32)
        im = np.ascontiguousarray(np.asarray(im).reshape(-1), dtype=np.int32)
        if q.shape[1] != self.d or px.shape != (q.shape[0], 2) or len(im) != len(s):
            raise IAError('ExactIndex.coherence: q (nq, %d), px (nq, 2) and len(s) == len(im) expected' % self.d)
        nq = q.shape[0]
        p = np.empty((nq, 2), dtype=np.int32)
        img = np.empty(nq, dtype=np.int32)
        rs = np.empty((nq, 2), dtype=np.int32)
        check(lib().ia_coherence_batch(self._h, _ptr(q), nq, _ptr(px), _ptr(s), _ptr(im), len(s), int(A_hw[0]),
                                       int(A_hw[1]), int(Bp_w), int(pad), _ptr(p), _ptr(img), _ptr(rs)),
              'ia_coherence_batch')
        return p, img, rs

    def close(self):
        if self._h:
            lib().ia_index_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ANN_MAX_LISTS = 4096  # IA_ANN_MAX_LISTS


def default_n_lists(n):
    """the lists of an AnnIndex over n rows when none are asked for: isqrt(n) clamped to 1..ANN_MAX_LISTS"""
    return max(1, min(ANN_MAX_LISTS, math.isqrt(int(n))))


def kmeans(ctx, pts, k, iters=5):
    """ia_kmeans: the deterministic Lloyd's k-means of include/ia.h (initial centre c = row floor(c n / k),
    ties to the lower centre, sums in ascending row order).  Returns (centers (k, d) float64, assign (n,)
    int32, iters_run)."""
    pts = _c64(pts)
    if pts.ndim != 2 or pts.shape[0] < 1:
        raise IAError('kmeans: pts must be a non-empty (n, d) array')
    n, d = pts.shape
    k = int(k)
    centers = np.empty((max(k, 0), d), dtype=np.float64)
    assign = np.empty(n, dtype=np.int32)
    run = ctypes.c_int()
    check(lib().ia_kmeans(ctx.handle, _ptr(pts), n, d, k, int(iters), _ptr(centers), _ptr(assign), ctypes.byref(run)),
          'ia_kmeans')
    return centers, assign, run.value


class AnnIndex(object):
    """ia_ann_*: the approximate index: k-means lists whose queries honour `checks`.
    n_lists = None: default_n_lists(n).  Deterministic; checks = -1 (or >= n) is ExactIndex.query_knn."""

    def __init__(self, ctx, pts, n_lists=None, iters=5):
        pts = _c64(pts)
        if pts.ndim != 2 or pts.shape[0] < 1:
            raise IAError('AnnIndex: pts must be a non-empty (n, d) array')
        self.ctx = ctx
        self.n, self.d = pts.shape
        self.n_lists = default_n_lists(self.n) if n_lists is None else int(n_lists)
        self._h = ctypes.c_void_p()
        check(lib().ia_ann_build(ctx.handle, _ptr(pts), self.n, self.d, self.n_lists, int(iters), ctypes.byref(self._h)),
              'ia_ann_build')

    def query(self, q, k=1, checks=32):
        """ia_ann_query: (idx (nq, k) int64, dist (nq, k) float64), shaped as ExactIndex.query_knn's"""
        q = _c64(np.atleast_2d(q))
        if q.shape[1] != self.d:
            raise IAError('AnnIndex.query: query width %d != index width %d' % (q.shape[1], self.d))
        k = int(k)
        idx = np.empty((q.shape[0], max(k, 0)), dtype=np.int64)
        dist = np.empty((q.shape[0], max(k, 0)), dtype=np.float64)
        check(lib().ia_ann_query(self._h, _ptr(q), q.shape[0], k, int(checks), _ptr(idx), _ptr(dist)), 'ia_ann_query')
        return idx, dist

    def lists(self):
        """ia_ann_lists: (centers (L, d) float64, sizes (L,) int64, rows (n,) int32: list after list, each ascending)"""
        centers = np.empty((self.n_lists, self.d), dtype=np.float64)
        sizes = np.empty(self.n_lists, dtype=np.int64)
        rows = np.empty(self.n, dtype=np.int32)
        check(lib().ia_ann_lists(self._h, _ptr(centers), _ptr(sizes), _ptr(rows)), 'ia_ann_lists')
        return centers, sizes, rows

    def stats(self):
        """ia_ann_stats: (rows whose distance the last query call computed, lists it probed - both summed over
        its queries -, k-means iterations of the build)"""
        out = (ctypes.c_int64 * 3)()
        check(lib().ia_ann_stats(self._h, out), 'ia_ann_stats')
        return int(out[0]), int(out[1]), int(out[2])

    def build_ms(self):
        """ia_ann_build_ms: host-clock ms of the build's (assign, grouping, update, list-major copy)"""
        out = (ctypes.c_double * 4)()
        check(lib().ia_ann_build_ms(self._h, out), 'ia_ann_build_ms')
        return tuple(float(v) for v in out)

    def close(self):
        if self._h:
            lib().ia_ann_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id():
    buf = ctypes.create_string_buffer(128)
    check(lib().ia_comm_unique_id(buf), 'ia_comm_unique_id')
    return buf.raw


def merge_winners(dist, row):
    """Host restatement-free merge (compiled in libia): dist/row (world, nq) -> (nq,) winners."""
    dist = _c64(dist)
    row = np.ascontiguousarray(row, dtype=np.int64)
    world, nq = dist.shape
    do = np.empty(nq, dtype=np.float64)
    ro = np.empty(nq, dtype=np.int64)
    check(lib().ia_merge_winners(_ptr(dist), _ptr(row), world, nq, _ptr(do), _ptr(ro)), 'ia_merge_winners')
    return do, ro


def wavefront_step(h, w, t):
    """(r0, M): step t covers pixels (r, t - 3r) for r in r0 .. r0 + M - 1."""
    r0, m = ctypes.c_int(), ctypes.c_int()
    check(lib().ia_wavefront_step(h, w, t, ctypes.byref(r0), ctypes.byref(m)), 'ia_wavefront_step')
    return r0.value, m.value


def wavefront_shape_pad(h, w, pad):
    """(steps, max_queries) of the schedule t = col + (pad + 1) row (include/ia.h ia_wavefront_shape_pad)"""
    s, m = ctypes.c_int64(), ctypes.c_int64()
    check(lib().ia_wavefront_shape_pad(h, w, pad, ctypes.byref(s), ctypes.byref(m)), 'ia_wavefront_shape_pad')
    return s.value, m.value


def wavefront_step_pad(h, w, pad, t):
    """(r0, M): step t covers pixels (r, t - (pad + 1) r) for r in r0 .. r0 + M - 1."""
    r0, m = ctypes.c_int(), ctypes.c_int()
    check(lib().ia_wavefront_step_pad(h, w, pad, t, ctypes.byref(r0), ctypes.byref(m)), 'ia_wavefront_step_pad')
    return r0.value, m.value


def masked_step_list(mask, pad):
    """ia_masked_step_list: (offsets (T + 1,), pixels (count,)) int32 for a 2-D bool / uint8 mask: the masked
    raster indices of step t of the schedule t = col + (pad + 1) row are pixels[offsets[t]:offsets[t + 1]]."""
    mask = np.array(mask, dtype=np.uint8, order='C')
    if mask.ndim != 2:
        raise IAError('masked_step_list: a 2-D mask expected')
    h, w = mask.shape
    offsets = np.zeros(max(w + (pad + 1) * (h - 1), 0) + 1, dtype=np.int32)
    pixels = np.zeros(max(int(np.count_nonzero(mask)), 1), dtype=np.int32)
    check(lib().ia_masked_step_list(h, w, int(pad), _ptr(mask), _ptr(offsets), _ptr(pixels)), 'ia_masked_step_list')
    return offsets, pixels[:int(offsets[-1])]


def shard_tiles(n_rows, world, rank):
    """Tiles [t0, t1) of `rank`; position j of tile t holds DB row j * ceil(n_rows/32) + t."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    check(lib().ia_shard_tiles(n_rows, world, rank, ctypes.byref(a), ctypes.byref(b)), 'ia_shard_tiles')
    return a.value, b.value


def shard_tiles_pruned(n_rows, world, rank):
    """Storage tiles [t0, t1) of `rank` on a pruned level (Morton tiles rank, rank + world, ...)."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    check(lib().ia_shard_tiles_pruned(n_rows, world, rank, ctypes.byref(a), ctypes.byref(b)), 'ia_shard_tiles_pruned')
    return a.value, b.value


def shard_morton_tile(storage_tile, n_tiles, world):
    return lib().ia_shard_morton_tile(storage_tile, n_tiles, world)


TILE_MUL = 2654435761  # IA_TILE_MUL of ia_internal.h


def shard_rows(n_rows, world, rank):
    """Sorted DB rows owned by `rank` (tile-strided layout, see shard_tiles)."""
    t0, t1 = shard_tiles(n_rows, world, rank)
    nt = (n_rows + 31) // 32
    perm = np.arange(t0, t1, dtype=np.int64) * (TILE_MUL % nt) % nt  # ia_tile_perm (ia_internal.h)
    rows = (np.arange(32)[:, None] * nt + perm[None, :]).ravel()
    return np.sort(rows[rows < n_rows])


def chain_budget(n_cu, vgprs, api_blocks_per_cu, wg_threads=64):
    """include/ia.h ia_chain_budget: deadlock-free handoff-chained waves in flight (0: never chain)"""
    return lib().ia_chain_budget(n_cu, vgprs, api_blocks_per_cu, wg_threads)


def chain_choice(level_waves, in_flight, budget, two_wave=1):
    """include/ia.h ia_chain_choice: 2 (two-wave workgroups, twice the waves reserved), 1 (one-wave) or 0 (unchained)"""
    return lib().ia_chain_choice(level_waves, in_flight, budget, two_wave)


def wavefront_shape(h, w):
    s, m = ctypes.c_int64(), ctypes.c_int64()
    check(lib().ia_wavefront_shape(h, w, ctypes.byref(s), ctypes.byref(m)), 'ia_wavefront_shape')
    return s.value, m.value
