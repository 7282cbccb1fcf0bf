"""ctypes binding of libkwmatch.so (include/kwmatch.h).

The library is built in-tree (``advanced_scrapper_amd/lib/``) by
``advanced_scrapper_amd.build`` / ``__graft_entry__.build()``.  There is no
fallback: if the library is missing or fails to load, every GPU entry point
raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib')
DEFAULT_LIB = os.path.join(LIB_DIR, 'libkwmatch.so')
LIB_PATH = DEFAULT_LIB


def _lib_path() -> str:
    """The default in-tree library; ``KW_LIB`` (a tuning variant of build.build_kwmatch_variant) only when
    ``bench.py --lib-variant`` asked for it (``KW_LIB_VARIANT_OK=1``): nothing else may swap the library."""
    alt = os.environ.get('KW_LIB')
    if not alt or os.path.abspath(alt) == DEFAULT_LIB:
        return DEFAULT_LIB
    if os.environ.get('KW_LIB_VARIANT_OK') != '1':
        raise RuntimeError(f"KW_LIB={alt}: only bench.py --lib-variant loads a non-default libkwmatch")
    return os.path.abspath(alt)

KW_OK = 0
KW_EINVAL = -1
KW_EUNSUPPORTED = -2
KW_EHIP = -3
KW_EOVERFLOW = -4
KW_ESTATE = -5
KW_NOPOS = 0xFFFFFFFF

HIT_DTYPE = np.dtype([('doc', '<u4'), ('pattern', '<u4'), ('pos', '<u4'), ('field', '<u4')])

# every symbol include/kwmatch.h, include/kwdedup.h, include/kwrows.h, include/kwingest.h and include/kwsort.h declare
EXPORTS = ('kw_compile', 'kw_scan', 'kw_hits', 'kw_hits_copy', 'kw_stats', 'kw_last_kernel_ms',
           'kw_last_kernel_times', 'kw_doc_routes', 'kw_scan_counts', 'kw_filter_variant', 'kw_last_error',
           'kw_destroy',
           'kw_scan_host', 'kw_hits_host', 'kw_device_count', 'kw_device_init',
           'kw_comm_unique_id', 'kw_comm_init', 'kw_allgather_counts', 'kw_allgather_hits',
           'kw_allgather_hits_planned', 'kw_exchange_plan', 'kw_exchange_caps_ok', 'kw_comm_last_error',
           'kw_comm_destroy',
           'kw_dedup_create', 'kw_dedup_run', 'kw_dedup_counts', 'kw_dedup_kept_size', 'kw_dedup_kept_copy',
           'kw_dedup_last_ms', 'kw_dedup_last_error', 'kw_dedup_destroy', 'dedup_urls',
           'kw_dedup_geometry', 'kw_dedup_route_counts',
           'kw_cdx_begin', 'kw_cdx_append', 'kw_cdx_rows', 'kw_cdx_store_copy', 'kw_cdx_run', 'kw_cdx_csv_size',
           'kw_cdx_csv_copy', 'kw_cdx_last_ms', 'kw_cdx_tile_bytes',
           'kw_csv_append', 'kw_cdx_run_exclude', 'kw_cdx_exclude_codes', 'kw_cdx_exclude_counts',
           'kw_cdx_remaining_size', 'kw_cdx_remaining_copy', 'kw_cdx_exclude_last_ms',
           'kw_cdx_run_exclude_unique', 'kw_cdx_exclude_duplicates', 'kw_cdx_selected_ts', 'kw_cdx_csv_select_size',
           'kw_cdx_csv_select_copy', 'kw_cdx_select_last_ms',
           'kw_csv_stream_begin', 'kw_csv_stream_window', 'kw_csv_stream_end', 'kw_cdx_exclude_distinct_seen',
           'kw_rows_create', 'kw_rows_run', 'kw_rows_copy', 'kw_rows_last_ms', 'kw_rows_last_error',
           'kw_rows_destroy',
           'kw_rows_cells', 'kw_rows_emit', 'kw_rows_emit_result', 'kw_rows_copy_index', 'kw_rows_emit_last_ms',
           'kw_rows_cells_device',
           'kw_ingest_create', 'kw_ingest_destroy', 'kw_ingest_last_error', 'kw_ingest_last_ms',
           'kw_ingest_tile_bytes', 'kw_ingest_parse', 'kw_ingest_cells', 'kw_ingest_arena', 'kw_ingest_dates',
           'kw_ingest_column_flags', 'kw_ingest_copy_cells', 'kw_ingest_copy_column', 'kw_ingest_stage',
           'kw_ingest_copy_arena', 'kw_ingest_dates_iso',
           'kw_ingest_upload', 'kw_ingest_spans', 'kw_ingest_copy_spans',
           'kw_ingest_zone', 'kw_ingest_stamps', 'kw_ingest_stamps_device', 'kw_rows_emit_stamps_device',
           'kw_sort_create', 'kw_sort_destroy', 'kw_sort_last_error', 'kw_sort_last_ms', 'kw_sort_keys',
           'kw_sort_gather', 'kw_sort_begin', 'kw_sort_window', 'kw_sort_finish', 'kw_sort_gather_begin',
           'kw_sort_gather_slab',
           'kw_sort_index_begin', 'kw_sort_index_stage', 'kw_sort_index_window', 'kw_sort_index_finish')

# KW_CDX_* verdicts of kw_cdx_append (include/kwdedup.h)
(KW_CDX_OK, KW_CDX_QUOTE, KW_CDX_CR, KW_CDX_NUL, KW_CDX_FIELDS, KW_CDX_TS, KW_CDX_URL, KW_CDX_UTF8,
 KW_CDX_HEADER) = range(9)


class CdxDialect(ctypes.Structure):
    """kw_cdx_dialect (include/kwdedup.h)."""
    _fields_ = [('delim', ctypes.c_uint8), ('ts_col', ctypes.c_int32), ('url_col', ctypes.c_int32),
                ('skip_lines', ctypes.c_int32), ('exact_fields', ctypes.c_int32)]

# KW_URL_* row codes (include/kwdedup.h)
KW_URL_NO_HTML, KW_URL_KEPT, KW_URL_FILTERED, KW_URL_DUPLICATE = 0, 1, 2, 3
KW_URL_SEEN = 5   # a link row of kw_cdx_run_exclude whose string is among the exclude rows
# KW_CSV_* verdicts of kw_csv_append (include/kwdedup.h), in the order they are tested
(KW_CSV_OK, KW_CSV_NUL, KW_CSV_UTF8, KW_CSV_HEADER, KW_CSV_QUOTE, KW_CSV_CR, KW_CSV_ROWS, KW_CSV_FIELDS,
 KW_CSV_URL) = range(9)
KW_DEDUP_NORMALIZE = 1
KW_ROWS_OK, KW_ROWS_INVALID_REGEX = 0, 1   # verdicts of kw_rows_run (include/kwrows.h)
KW_EMIT_OK, KW_EMIT_NUL = 0, 1             # verdicts of kw_rows_emit (include/kwrows.h)
# KW_INGEST_* verdicts of kw_ingest_parse (include/kwingest.h), in the order they are tested
(KW_INGEST_OK, KW_INGEST_NUL, KW_INGEST_UTF8, KW_INGEST_QUOTE, KW_INGEST_CR, KW_INGEST_BLANK, KW_INGEST_FIELDS,
 KW_INGEST_ROWS) = range(8)
# KW_SORT_* verdicts of kw_sort_keys (include/kwsort.h), in the order they are tested
KW_SORT_OK, KW_SORT_KEY, KW_SORT_FORM, KW_SORT_DTYPE = range(4)
KW_INDEX_OK, KW_INDEX_TERM = 0, 1          # verdicts of kw_sort_index_finish (include/kwsort.h)
KW_N_STATS = 21
# KW_RESCAN_* bits of stats[20] (include/kwmatch.h)
KW_RESCAN_GENERIC_ITEMS, KW_RESCAN_RESULTS, KW_RESCAN_GENERIC_CPS = 1, 2, 4
KW_RESCAN_REGEX_QUEUE, KW_RESCAN_TASK_QUEUES, KW_RESCAN_DECIDED_SET, KW_RESCAN_REGIONS = 16, 32, 64, 128
KW_COMM_ID_BYTES = 128
KW_ROUTE_SCAN, KW_ROUTE_RESOLVE, KW_ROUTE_GENERIC, KW_ROUTE_TRANSCODE = 0, 1, 2, 3
KW_PLAN_SEND, KW_PLAN_RECV = 1, 2


class KwError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libkwmatch error {code}: {msg}")
        self.code = code


_LIB = None


def lib() -> ctypes.CDLL:
    """Load libkwmatch.so (raises if it was not built)."""
    global _LIB, LIB_PATH
    if _LIB is not None:
        return _LIB
    LIB_PATH = _lib_path()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.kw_dedup_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.kw_dedup_run.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    L.kw_dedup_counts.argtypes = [vp, vp]
    L.kw_dedup_kept_size.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.kw_dedup_kept_copy.argtypes = [vp, vp, vp, vp, vp]
    L.kw_dedup_last_ms.argtypes = [vp, vp, i32]
    L.kw_dedup_last_error.argtypes = [vp]
    L.kw_dedup_last_error.restype = ctypes.c_char_p
    L.kw_dedup_destroy.argtypes = [vp]
    L.dedup_urls.argtypes = [vp, vp, i64, vp, vp]
    L.kw_dedup_geometry.argtypes = [vp, i32]
    L.kw_dedup_route_counts.argtypes = [vp, vp, i32]
    for f in ('kw_dedup_create', 'kw_dedup_run', 'kw_dedup_counts', 'kw_dedup_kept_size', 'kw_dedup_kept_copy',
              'kw_dedup_last_ms', 'kw_dedup_destroy', 'dedup_urls', 'kw_dedup_geometry', 'kw_dedup_route_counts'):
        getattr(L, f).restype = ctypes.c_int
    L.kw_cdx_begin.argtypes = [vp]
    L.kw_cdx_append.argtypes = [vp, vp, i64, ctypes.POINTER(CdxDialect), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                ctypes.POINTER(i64), vp]
    L.kw_cdx_rows.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.kw_cdx_store_copy.argtypes = [vp, vp, vp, vp, vp]
    L.kw_cdx_run.argtypes = [vp, i32, vp]
    L.kw_cdx_csv_size.argtypes = [vp, ctypes.POINTER(i64), vp]
    L.kw_cdx_csv_copy.argtypes = [vp, vp, vp]
    L.kw_cdx_last_ms.argtypes = [vp, vp, i32]
    L.kw_cdx_tile_bytes.argtypes = []
    for f in ('kw_cdx_begin', 'kw_cdx_append', 'kw_cdx_rows', 'kw_cdx_store_copy', 'kw_cdx_run', 'kw_cdx_csv_size',
              'kw_cdx_csv_copy', 'kw_cdx_last_ms', 'kw_cdx_tile_bytes'):
        getattr(L, f).restype = ctypes.c_int
    L.kw_csv_append.argtypes = [vp, vp, i64, ctypes.c_char_p, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i32),
                                ctypes.POINTER(i64), vp]
    L.kw_cdx_run_exclude.argtypes = [vp, i64, vp]
    L.kw_cdx_exclude_codes.argtypes = [vp, vp, vp]
    L.kw_cdx_exclude_counts.argtypes = [vp, vp]
    L.kw_cdx_remaining_size.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.kw_cdx_remaining_copy.argtypes = [vp, vp, vp, vp, vp]
    L.kw_cdx_exclude_last_ms.argtypes = [vp, vp, i32]
    for f in ('kw_csv_append', 'kw_cdx_run_exclude', 'kw_cdx_exclude_codes', 'kw_cdx_exclude_counts',
              'kw_cdx_remaining_size', 'kw_cdx_remaining_copy', 'kw_cdx_exclude_last_ms'):
        getattr(L, f).restype = ctypes.c_int
    L.kw_cdx_run_exclude_unique.argtypes = [vp, i64, vp]
    L.kw_cdx_exclude_duplicates.argtypes = [vp, ctypes.POINTER(i64)]
    L.kw_cdx_selected_ts.argtypes = [vp, vp, vp]
    L.kw_cdx_csv_select_size.argtypes = [vp, vp, i64, vp, i64, vp, ctypes.POINTER(i64), vp]
    L.kw_cdx_csv_select_copy.argtypes = [vp, vp, vp]
    L.kw_cdx_select_last_ms.argtypes = [vp, vp, i32]
    for f in ('kw_cdx_run_exclude_unique', 'kw_cdx_exclude_duplicates', 'kw_cdx_selected_ts', 'kw_cdx_csv_select_size',
              'kw_cdx_csv_select_copy', 'kw_cdx_select_last_ms'):
        getattr(L, f).restype = ctypes.c_int
    L.kw_csv_stream_begin.argtypes = [vp, ctypes.c_char_p, i32, i32]
    L.kw_csv_stream_window.argtypes = [vp, vp, i64, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                       ctypes.POINTER(i64), vp]
    L.kw_csv_stream_end.argtypes = [vp, i32, ctypes.POINTER(i64)]
    L.kw_cdx_exclude_distinct_seen.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    for f in ('kw_csv_stream_begin', 'kw_csv_stream_window', 'kw_csv_stream_end', 'kw_cdx_exclude_distinct_seen'):
        getattr(L, f).restype = ctypes.c_int
    L.kw_rows_create.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, ctypes.POINTER(vp)]
    L.kw_rows_run.argtypes = [vp, vp, i64, vp, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i64),
                              ctypes.POINTER(i32), vp]
    L.kw_rows_copy.argtypes = [vp, vp, vp, vp, vp]
    L.kw_rows_last_ms.argtypes = [vp, vp, i32]
    L.kw_rows_destroy.argtypes = [vp]
    L.kw_rows_cells.argtypes = [vp, vp, vp, vp, i64, i32, vp]
    L.kw_rows_emit.argtypes = [vp, vp, vp, i64, i64, ctypes.POINTER(i64), ctypes.POINTER(i32), vp]
    L.kw_rows_emit_result.argtypes = [vp] + [ctypes.POINTER(vp)] * 6
    L.kw_rows_copy_index.argtypes = [vp, vp, vp]
    L.kw_rows_emit_last_ms.argtypes = [vp, vp, i32]
    for f in ('kw_rows_create', 'kw_rows_run', 'kw_rows_copy', 'kw_rows_last_ms', 'kw_rows_destroy', 'kw_rows_cells',
              'kw_rows_emit', 'kw_rows_emit_result', 'kw_rows_copy_index', 'kw_rows_emit_last_ms'):
        getattr(L, f).restype = ctypes.c_int
    L.kw_rows_cells_device.argtypes = [vp, vp, vp, vp, i64, i32, vp]
    L.kw_rows_cells_device.restype = ctypes.c_int
    L.kw_ingest_create.argtypes = [i32, i32, vp, vp, vp, i32, ctypes.POINTER(vp)]
    L.kw_ingest_destroy.argtypes = [vp]
    L.kw_ingest_last_ms.argtypes = [vp, vp, i32]
    L.kw_ingest_tile_bytes.argtypes = []
    L.kw_ingest_parse.argtypes = [vp, vp, i64, i32, i64, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                  ctypes.POINTER(i64), vp]
    L.kw_ingest_cells.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i64)]
    L.kw_ingest_arena.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i64)]
    L.kw_ingest_dates.argtypes = [vp, vp, vp]
    L.kw_ingest_dates_iso.argtypes = [vp, vp, vp, vp]
    L.kw_ingest_dates_iso.restype = ctypes.c_int
    L.kw_ingest_column_flags.argtypes = [vp, vp]
    L.kw_ingest_copy_cells.argtypes = [vp, vp, vp, vp]
    L.kw_ingest_copy_column.argtypes = [vp, i32, vp, i64, vp, vp]
    L.kw_ingest_stage.argtypes = [vp, i32, i64, ctypes.POINTER(vp)]
    L.kw_ingest_upload.argtypes = [vp, i32, i64, i64, ctypes.POINTER(vp), vp]
    L.kw_ingest_copy_arena.argtypes = [vp, vp, vp]
    for f in ('kw_ingest_create', 'kw_ingest_destroy', 'kw_ingest_last_ms', 'kw_ingest_tile_bytes', 'kw_ingest_parse',
              'kw_ingest_stage', 'kw_ingest_upload', 'kw_ingest_cells', 'kw_ingest_arena', 'kw_ingest_dates',
              'kw_ingest_column_flags', 'kw_ingest_copy_cells', 'kw_ingest_copy_arena', 'kw_ingest_copy_column'):
        getattr(L, f).restype = ctypes.c_int
    L.kw_ingest_last_error.argtypes = [vp]
    L.kw_ingest_last_error.restype = ctypes.c_char_p
    L.kw_ingest_spans.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                  ctypes.POINTER(vp), ctypes.POINTER(i64)]
    L.kw_ingest_copy_spans.argtypes = [vp, vp, vp]
    L.kw_ingest_zone.argtypes = [vp, vp, vp, i32]
    L.kw_ingest_stamps.argtypes = [vp, vp, vp]
    L.kw_ingest_stamps_device.argtypes = [vp, ctypes.POINTER(vp)]
    L.kw_rows_emit_stamps_device.argtypes = [vp, vp, vp, i64, i64, ctypes.POINTER(i64), ctypes.POINTER(i32), vp]
    for f in ('kw_ingest_zone', 'kw_ingest_stamps', 'kw_ingest_stamps_device', 'kw_rows_emit_stamps_device'):
        getattr(L, f).restype = ctypes.c_int
    L.kw_sort_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.kw_sort_destroy.argtypes = [vp]
    L.kw_sort_keys.argtypes = [vp, vp, i32, i64, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i64),
                               ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(i32), vp]
    L.kw_sort_gather.argtypes = [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(i64)]
    L.kw_sort_last_ms.argtypes = [vp, vp, i32]
    L.kw_sort_begin.argtypes = [vp, i32, i64, i64]
    L.kw_sort_window.argtypes = [vp, vp, i64, vp]
    L.kw_sort_finish.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                 ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.kw_sort_gather_begin.argtypes = [vp, vp, i64, i64, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.kw_sort_gather_slab.argtypes = [vp, i64, ctypes.POINTER(vp), ctypes.POINTER(i64)]
    L.kw_sort_index_begin.argtypes = [vp, vp, i64, i64, ctypes.POINTER(i64)]
    L.kw_sort_index_stage.argtypes = [vp, i32, i64, ctypes.POINTER(vp)]
    L.kw_sort_index_window.argtypes = [vp, i32, i64, vp]
    L.kw_sort_index_finish.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i64)]
    for f in ('kw_ingest_spans', 'kw_ingest_copy_spans', 'kw_sort_create', 'kw_sort_destroy', 'kw_sort_keys',
              'kw_sort_gather', 'kw_sort_last_ms', 'kw_sort_begin', 'kw_sort_window', 'kw_sort_finish',
              'kw_sort_gather_begin', 'kw_sort_gather_slab', 'kw_sort_index_begin', 'kw_sort_index_stage',
              'kw_sort_index_window', 'kw_sort_index_finish'):
        getattr(L, f).restype = ctypes.c_int
    L.kw_sort_last_error.argtypes = [vp]
    L.kw_sort_last_error.restype = ctypes.c_char_p
    L.kw_rows_last_error.argtypes = [vp]
    L.kw_rows_last_error.restype = ctypes.c_char_p
    L.kw_compile.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, i64, i32, ctypes.POINTER(vp)]
    L.kw_compile.restype = ctypes.c_int
    L.kw_scan.argtypes = [vp, vp, vp, i64, vp]
    L.kw_scan.restype = ctypes.c_int
    L.kw_hits.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(vp)]
    L.kw_hits.restype = ctypes.c_int
    L.kw_hits_copy.argtypes = [vp, vp, i64, ctypes.POINTER(i64), vp]
    L.kw_hits_copy.restype = ctypes.c_int
    L.kw_stats.argtypes = [vp, vp, i32]
    L.kw_stats.restype = ctypes.c_int
    L.kw_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                    ctypes.POINTER(ctypes.c_float)]
    L.kw_last_kernel_ms.restype = ctypes.c_int
    L.kw_last_kernel_times.argtypes = [vp, vp, i32]
    L.kw_last_kernel_times.restype = ctypes.c_int
    L.kw_doc_routes.argtypes = [vp, vp, i64]
    L.kw_doc_routes.restype = ctypes.c_int
    if hasattr(L, 'kw_filter_variant'):   # (as kw_scan_counts below)
        L.kw_filter_variant.argtypes = [vp, vp]
        L.kw_filter_variant.restype = ctypes.c_int
    if hasattr(L, 'kw_scan_counts'):   # (a tuning variant built from an earlier tree, for an A/B, has none)
        L.kw_scan_counts.argtypes = [vp, vp, i64, vp, i32]
        L.kw_scan_counts.restype = ctypes.c_int
    L.kw_scan_host.argtypes = [vp, vp, i64, vp, i64]
    L.kw_scan_host.restype = ctypes.c_int
    L.kw_hits_host.argtypes = [vp, vp, i64, ctypes.POINTER(i64)]
    L.kw_hits_host.restype = ctypes.c_int
    L.kw_device_count.argtypes = [ctypes.POINTER(i32)]
    L.kw_device_count.restype = ctypes.c_int
    L.kw_device_init.argtypes = [i32]
    L.kw_device_init.restype = ctypes.c_int
    L.kw_comm_unique_id.argtypes = [vp]
    L.kw_comm_init.argtypes = [i32, i32, vp, i32, ctypes.POINTER(vp)]
    L.kw_allgather_counts.argtypes = [vp, i64, vp, vp]
    L.kw_allgather_hits.argtypes = [vp, vp, i64, i64, i32, vp, i64, ctypes.POINTER(i64), vp, vp]
    L.kw_allgather_hits_planned.argtypes = [vp, vp, i64, i64, i32, vp, vp, i64, ctypes.POINTER(i64), vp]
    L.kw_exchange_caps_ok.argtypes = [i32, i32, vp, vp, ctypes.POINTER(i32)]
    L.kw_exchange_caps_ok.restype = ctypes.c_int
    L.kw_comm_destroy.argtypes = [vp]
    L.kw_exchange_plan.argtypes = [i32, i32, i32, vp, vp, vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.kw_exchange_plan.restype = ctypes.c_int
    for f in ('kw_comm_unique_id', 'kw_comm_init', 'kw_allgather_counts', 'kw_allgather_hits',
              'kw_allgather_hits_planned', 'kw_comm_destroy'):
        getattr(L, f).restype = ctypes.c_int
    L.kw_comm_last_error.argtypes = [vp]
    L.kw_comm_last_error.restype = ctypes.c_char_p
    L.kw_last_error.argtypes = [vp]
    L.kw_last_error.restype = ctypes.c_char_p
    L.kw_destroy.argtypes = [vp]
    L.kw_destroy.restype = ctypes.c_int
    _LIB = L
    return L


def lib_identity() -> dict:
    """Which libkwmatch this process loaded: path (relative to the package), sha256, default or variant."""
    import hashlib
    lib()
    with open(LIB_PATH, 'rb') as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()
    return {'path': os.path.relpath(LIB_PATH, os.path.dirname(LIB_DIR)), 'sha256': digest,
            'default': LIB_PATH == DEFAULT_LIB,
            'env': {k: v for k, v in sorted(os.environ.items()) if k.startswith('KW_')}}


def device_count() -> int:
    """HIP devices visible to this process (libkwmatch's hipGetDeviceCount; no torch)."""
    n = ctypes.c_int32()
    lib().kw_device_count(ctypes.byref(n))
    return int(n.value)


def exchange_plan(nranks: int, rank: int, root: int, counts):
    """kw_exchange_plan (pure host): (recv_off[nranks + 1], ops[nranks], n_total, n_recv) of `rank`."""
    cnt = np.ascontiguousarray(counts, dtype=np.int64)
    off = np.zeros(nranks + 1, dtype=np.int64)
    ops = np.zeros(nranks, dtype=np.int32)
    tot, nrecv = ctypes.c_int64(), ctypes.c_int64()
    rc = lib().kw_exchange_plan(nranks, rank, root, ptr(cnt), ptr(off), ptr(ops), ctypes.byref(tot), ctypes.byref(nrecv))
    if rc != KW_OK:
        raise KwError(rc, 'kw_exchange_plan: bad arguments')
    return off, ops, int(tot.value), int(nrecv.value)


def exchange_caps_ok(nranks: int, root: int, counts, caps):
    """kw_exchange_caps_ok (pure host): (ok, first short receiver or -1)."""
    cnt = np.ascontiguousarray(counts, dtype=np.int64)
    cap = np.ascontiguousarray(caps, dtype=np.int64)
    bad = ctypes.c_int32(-1)
    rc = lib().kw_exchange_caps_ok(nranks, root, ptr(cnt), ptr(cap), ctypes.byref(bad))
    if rc not in (KW_OK, KW_EOVERFLOW):
        raise KwError(rc, 'kw_exchange_caps_ok: bad arguments')
    return rc == KW_OK, int(bad.value)


def check(rc: int, handle=None) -> None:
    if rc != KW_OK:
        msg = lib().kw_last_error(handle)
        raise KwError(rc, msg.decode('utf-8', 'replace') if msg else '')


def check_comm(rc: int, comm=None) -> None:
    if rc != KW_OK:
        msg = lib().kw_comm_last_error(comm)
        raise KwError(rc, msg.decode('utf-8', 'replace') if msg else '')


def ptr(a) -> ctypes.c_void_p:
    """Raw pointer of a numpy array or torch tensor."""
    if a is None:
        return ctypes.c_void_p(0)
    if isinstance(a, np.ndarray):
        return ctypes.c_void_p(a.ctypes.data)
    return ctypes.c_void_p(a.data_ptr())
