"""ctypes binding of the C ABI in include/zippy_hip.h.

`Engine(lib_path)` wraps one zh_ctx.  The product entry point (zippy_amd.api)
always passes zippy_amd/libzippy_hip.so; the test-suite also points this class at
the g++/emulator build of the same sources (tests/hipemu) to check kernel logic
without a GPU.  There is no fallback between the two.
"""
import ctypes
import os

from .common import ZippyError, dfDetect, dfGzip, BestSpeed, DefaultCompression

_c = ctypes
_SIGS = {
    "zh_create": (_c.c_int, [_c.c_int, _c.c_void_p, _c.POINTER(_c.c_void_p)]),
    "zh_destroy": (None, [_c.c_void_p]),
    "zh_strerror": (_c.c_char_p, [_c.c_int]),
    "zh_last_error": (_c.c_char_p, [_c.c_void_p]),
    "zh_stream": (_c.c_void_p, [_c.c_void_p]),
    "zh_set_gzip_fname_len": (None, [_c.c_void_p, _c.c_int]),
    "zh_set_host_pipeline": (None, [_c.c_void_p, _c.c_size_t, _c.c_size_t]),
    "zh_chain_links_parallel": (_c.c_int, [_c.c_void_p]),
    "zh_set_inflate_mode": (None, [_c.c_void_p, _c.c_int]),
    "zh_set_l1_parse": (None, [_c.c_void_p, _c.c_int]),
    "zh_compress_bound": (_c.c_size_t, [_c.c_size_t, _c.c_int]),
    "zh_compress_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                     _c.c_size_t, _c.c_int, _c.c_int, _c.POINTER(_c.c_void_p),
                                     _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32)]),
    "zh_compress_batch_into": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                          _c.c_size_t, _c.c_int, _c.c_int, _c.POINTER(_c.c_void_p),
                                          _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_size_t),
                                          _c.POINTER(_c.c_int32)]),
    "zh_uncompress_batch_into": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                            _c.c_size_t, _c.c_int, _c.POINTER(_c.c_void_p),
                                            _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_size_t),
                                            _c.POINTER(_c.c_int32)]),
    "zh_uncompress_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p),
                                       _c.POINTER(_c.c_size_t), _c.c_size_t, _c.c_int,
                                       _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                       _c.POINTER(_c.c_int32)]),
    "zh_device_count": (_c.c_int, []),
    "zh_compress_batch_multi": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_size_t, _c.POINTER(_c.c_void_p),
                                           _c.POINTER(_c.c_size_t), _c.c_size_t, _c.c_int, _c.c_int,
                                           _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                           _c.POINTER(_c.c_int32)]),
    "zh_uncompress_batch_multi": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_size_t, _c.POINTER(_c.c_void_p),
                                             _c.POINTER(_c.c_size_t), _c.c_size_t, _c.c_int,
                                             _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                             _c.POINTER(_c.c_int32)]),
    "zh_compress": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int,
                               _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t)]),
    "zh_uncompress": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int,
                                 _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t)]),
    "zh_crc32": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_uint32)]),
    "zh_adler32": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_uint32)]),
    "zh_free": (None, [_c.c_void_p]),
    "zh_device_malloc": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_void_p)]),
    "zh_device_free": (None, [_c.c_void_p, _c.c_void_p]),
    "zh_device_upload": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t]),
    "zh_device_download": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t]),
    "zh_plan_compress": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_uint64),
                                    _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                    _c.POINTER(_c.c_uint64), _c.c_int, _c.c_int,
                                    _c.POINTER(_c.c_void_p)]),
    "zh_plan_uncompress": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_uint64),
                                      _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                      _c.POINTER(_c.c_uint64), _c.c_int, _c.POINTER(_c.c_void_p)]),
    "zh_plan_run": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "zh_plan_results": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_int32)]),
    "zh_plan_device_lens": (_c.c_void_p, [_c.c_void_p]),
    "zh_plan_device_statuses": (_c.c_void_p, [_c.c_void_p]),
    "zh_plan_set_src_lens_device": (_c.c_int, [_c.c_void_p, _c.c_void_p]),
    "zh_plan_pack": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p]),
    "zh_plan_unpack": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "zh_plan_destroy": (None, [_c.c_void_p]),
    "zh_plan_set_profiling": (None, [_c.c_void_p, _c.c_int]),
    "zh_plan_kernel_times": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_char_p),
                                        _c.POINTER(_c.c_float), _c.c_int]),
    "zh_compress_blocks": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int,
                                      _c.c_size_t, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                      _c.POINTER(_c.POINTER(_c.c_uint64)), _c.POINTER(_c.c_size_t)]),
    "zh_uncompress_indexed": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int,
                                         _c.POINTER(_c.c_uint64), _c.c_size_t,
                                         _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t)]),
    "zh_plan_compress_blocks": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_uint64),
                                           _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                           _c.POINTER(_c.c_uint64), _c.c_int, _c.c_int, _c.c_size_t,
                                           _c.POINTER(_c.c_void_p)]),
    "zh_plan_block_index": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.POINTER(_c.c_uint64)),
                                       _c.POINTER(_c.c_size_t)]),
    "zh_plan_uncompress_indexed": (_c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_uint64,
                                              _c.c_uint64, _c.c_int, _c.POINTER(_c.c_uint64),
                                              _c.c_size_t, _c.POINTER(_c.c_void_p)]),
    "zh_plan_uncompress_ranges": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                             _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                             _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                             _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_void_p)]),
    "zh_uncompress_ranges": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                        _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                        _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                        _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32)]),
    "zh_debug_range_stats": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                        _c.POINTER(_c.c_uint64)]),
    "zh_bgzf_write_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                       _c.c_int, _c.c_size_t, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                       _c.POINTER(_c.c_int32)]),
    "zh_bgzf_read_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                      _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32),
                                      _c.POINTER(_c.c_uint8)]),
    "zh_bgzf_index_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                       _c.POINTER(_c.POINTER(_c.c_uint64)), _c.POINTER(_c.c_size_t),
                                       _c.POINTER(_c.c_int32), _c.POINTER(_c.c_uint8)]),
    "zh_bgzf_read_ranges": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                       _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                       _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                       _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32)]),
    "zh_gzip_read_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                      _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32),
                                      _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t)]),
    "zh_debug_gzip_stats": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                       _c.POINTER(_c.c_uint64)]),
    "zh_seek_index_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                       _c.c_int, _c.c_uint64, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                       _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32)]),
    "zh_seek_read_ranges": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                       _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                       _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64),
                                       _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32)]),
    "zh_uncompress_resume_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                              _c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                              _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint8),
                                              _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_size_t),
                                              _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32),
                                              _c.POINTER(_c.c_int32)]),
    "zh_compress_stream_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                            _c.c_int, _c.c_int, _c.c_size_t, _c.POINTER(_c.c_void_p),
                                            _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_uint8),
                                            _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_void_p),
                                            _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32)]),
    "zh_crc32_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                  _c.POINTER(_c.c_uint32)]),
    "zh_compress_batch_crc32": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                           _c.c_size_t, _c.c_int, _c.c_int, _c.POINTER(_c.c_void_p),
                                           _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32),
                                           _c.POINTER(_c.c_uint32)]),
    "zh_uncompress_batch_sized": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                             _c.c_size_t, _c.c_int, _c.POINTER(_c.c_uint64),
                                             _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                             _c.POINTER(_c.c_int32), _c.POINTER(_c.c_uint32)]),
    "zh_plan_request_crc32": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "zh_plan_crc32": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint32)]),
    "zh_zip_open": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_void_p)]),
    "zh_zip_close": (None, [_c.c_void_p]),
    "zh_zip_num_entries": (_c.c_size_t, [_c.c_void_p]),
    "zh_zip_entry_at": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "zh_zip_find": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "zh_zip_extract_batch": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_size_t), _c.c_size_t,
                                        _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                        _c.POINTER(_c.c_int32)]),
    "zh_zip_open_all_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                         _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_int32)]),
    "zh_zip_read_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                     _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_int32)]),
    "zh_zip_entry_v1": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_uint16), _c.POINTER(_c.c_uint16),
                                   _c.POINTER(_c.c_int)]),
    "zh_zip_data": (_c.c_void_p, [_c.c_void_p, _c.POINTER(_c.c_size_t)]),
    "zh_zip_entry_data": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                     _c.POINTER(_c.c_int32)]),
    "zh_zip_create": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_char_p), _c.POINTER(_c.c_size_t),
                                 _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                 _c.c_uint16, _c.c_uint16, _c.POINTER(_c.c_void_p),
                                 _c.POINTER(_c.c_size_t)]),
    "zh_tar_open": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_void_p)]),
    "zh_tar_close": (None, [_c.c_void_p]),
    "zh_tar_num_entries": (_c.c_size_t, [_c.c_void_p]),
    "zh_tar_entry_at": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "zh_tar_data": (_c.c_void_p, [_c.c_void_p, _c.POINTER(_c.c_size_t)]),
    "zh_tar_open_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.c_size_t,
                                     _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_int32)]),
    "zh_tar_read_batch": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                     _c.POINTER(_c.c_int32), _c.c_size_t, _c.POINTER(_c.c_void_p),
                                     _c.POINTER(_c.c_int32)]),
    "zh_tar_create_batch": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_size_t), _c.c_size_t, _c.c_int,
                                       _c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                       _c.POINTER(_c.c_int32)]),
    "zh_zip_write_batch": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_size_t), _c.c_size_t, _c.c_int,
                                      _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32)]),
    "zh_zip_create_batch": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_size_t), _c.c_size_t, _c.c_int,
                                       _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int32)]),
    "zh_debug_tokens": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int,
                                   _c.POINTER(_c.POINTER(_c.c_uint16)), _c.POINTER(_c.c_size_t)]),
    "zh_debug_huffman": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint32), _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                    _c.POINTER(_c.c_uint16), _c.POINTER(_c.c_uint8), _c.POINTER(_c.c_int)]),
    "zh_debug_segment_stats": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)  # every entry point include/zippy_hip.h declares


class GzipMember(_c.Structure):
    """zh_gzip_member (include/zippy_hip.h)"""
    _fields_ = [("coff", _c.c_uint64), ("cdata_off", _c.c_uint64), ("cdata_len", _c.c_uint64),
                ("uoff", _c.c_uint64), ("ulen", _c.c_uint64),
                ("crc", _c.c_uint32), ("isize", _c.c_uint32), ("mtime", _c.c_uint32),
                ("flg", _c.c_uint8), ("xfl", _c.c_uint8), ("os", _c.c_uint8), ("pad", _c.c_uint8),
                ("extra_off", _c.c_uint32), ("extra_len", _c.c_uint32), ("name_off", _c.c_uint32),
                ("name_len", _c.c_uint32), ("comment_off", _c.c_uint32), ("comment_len", _c.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "pad"}


def load_library(path):
    if not os.path.exists(path):
        raise ImportError(
            "%s is missing: build it with `python -m zippy_amd.build` (hipcc, gfx950). "
            "zippy_amd has no CPU fallback." % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def _u64(seq):
    arr = (_c.c_uint64 * len(seq))(*[int(x) for x in seq])
    return arr


class Plan:
    """A zh_plan: device-resident batch geometry (include/zippy_hip.h)."""

    def __init__(self, engine, handle, n):
        self.engine, self._h, self.n = engine, handle, n

    def run(self, d_src, d_dst):
        self.engine._check(self.engine.lib.zh_plan_run(self._h, d_src, d_dst))

    def results(self):
        lens = (_c.c_uint64 * self.n)()
        sts = (_c.c_int32 * self.n)()
        self.engine._check(self.engine.lib.zh_plan_results(self._h, lens, sts))
        return list(lens), list(sts)

    def block_index(self, buf=0):
        """[(bit_off, out_off), ...] of buffer `buf` of a compress plan (zh_plan_block_index)."""
        idx = _c.POINTER(_c.c_uint64)()
        n = _c.c_size_t()
        self.engine._check(self.engine.lib.zh_plan_block_index(self._h, buf, _c.byref(idx), _c.byref(n)))
        try:
            return [(idx[2 * i], idx[2 * i + 1]) for i in range(n.value)]
        finally:
            self.engine.lib.zh_free(idx)

    def device_lens(self):
        return self.engine.lib.zh_plan_device_lens(self._h)

    def device_statuses(self):
        """Device pointer of the n int32 statuses (zh_plan_device_statuses); valid after run."""
        return self.engine.lib.zh_plan_device_statuses(self._h)

    def request_crc32(self, on=True):
        """CRC-32 of the uncompressed side of every buffer, whatever the container: before run (zh_plan_request_crc32)."""
        self.engine._check(self.engine.lib.zh_plan_request_crc32(self._h, 1 if on else 0))

    def crc32(self):
        """The n CRC-32s requested with request_crc32, after run (zh_plan_crc32)."""
        crcs = (_c.c_uint32 * max(1, self.n))()
        if self.n:
            self.engine._check(self.engine.lib.zh_plan_crc32(self._h, crcs))
        return list(crcs)[:self.n]

    def set_src_lens_device(self, d_lens):
        self.engine._check(self.engine.lib.zh_plan_set_src_lens_device(self._h, d_lens))

    def pack(self, d_slots, d_packed, packed_cap, d_offsets):
        """The plan's results back to back at d_packed, n + 1 device uint64 offsets at d_offsets (zh_plan_pack)."""
        self.engine._check(self.engine.lib.zh_plan_pack(self._h, d_slots, d_packed, packed_cap, d_offsets))

    def unpack(self, d_packed, d_offsets, d_slots):
        """Streams back to back -> an uncompress plan's source slots and device-side lengths (zh_plan_unpack)."""
        self.engine._check(self.engine.lib.zh_plan_unpack(self._h, d_packed, d_offsets, d_slots))

    def set_profiling(self, on=True):
        self.engine.lib.zh_plan_set_profiling(self._h, 1 if on else 0)

    def kernel_times(self):
        names = (_c.c_char_p * 32)()
        ms = (_c.c_float * 32)()
        k = self.engine.lib.zh_plan_kernel_times(self._h, names, ms, 32)
        return [(names[i].decode(), ms[i]) for i in range(k)]

    def close(self):
        if self._h:
            self.engine.lib.zh_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ZipEntry(_c.Structure):
    _fields_ = [("path", _c.c_void_p), ("path_len", _c.c_size_t), ("is_directory", _c.c_int),
                ("header_offset", _c.c_uint64), ("compressed_size", _c.c_uint64),
                ("uncompressed_size", _c.c_uint64), ("crc32", _c.c_uint32), ("unix_mode", _c.c_uint32)]


class ZipReader:
    """zh_zip_reader over a bytes image: the ZipArchiveReader of ziparchives.nim:27-29."""

    def __init__(self, engine, image, handle=None):
        """handle: a reader zh_zip_open_all_batch made of `image` (Engine.open_zips); None: zh_zip_open"""
        self.engine = engine
        self._image = bytes(image)  # borrowed by the library until close
        h = _c.c_void_p()
        if handle is None:
            engine._check(engine.lib.zh_zip_open(self._image, len(self._image), _c.byref(h)))
        else:
            h = _c.c_void_p(handle)
        self._h = h
        self.entries = []
        for i in range(engine.lib.zh_zip_num_entries(h)):
            e = ZipEntry()
            engine._check(engine.lib.zh_zip_entry_at(h, i, _c.byref(e)))
            self.entries.append({
                "path": _c.string_at(e.path, e.path_len).decode("utf-8", "surrogateescape"),
                "is_directory": bool(e.is_directory), "header_offset": e.header_offset,
                "compressed_size": e.compressed_size, "uncompressed_size": e.uncompressed_size,
                "crc32": e.crc32, "unix_mode": e.unix_mode})

    def walk_files(self):
        return [e["path"] for e in self.entries if not e["is_directory"]]

    @property
    def data(self):
        """zh_zip_data: the block of extracted files of a reader made by Engine.open_zips (b"" otherwise)"""
        n = _c.c_size_t()
        base = self.engine.lib.zh_zip_data(self._h, _c.byref(n))
        return _c.string_at(base, n.value) if base and n.value else b""

    def _entry_data(self, i):
        data, n, st = _c.c_void_p(), _c.c_size_t(), _c.c_int32()
        self.engine._check(self.engine.lib.zh_zip_entry_data(self._h, i, _c.byref(data), _c.byref(n), _c.byref(st)))
        return data.value, n.value, st.value

    def entry_status(self, i):
        """zh_zip_entry_data's status of record i (a reader made by Engine.open_zips)"""
        return self._entry_data(i)[2]

    def contents(self, i):
        """the extracted bytes of record i, None unless its status is 0"""
        data, n, st = self._entry_data(i)
        if st:
            return None
        return _c.string_at(data, n) if n else b""

    def entry_v1(self, i):
        """zh_zip_entry_v1: (dos_time, dos_date, in_directory) of entry i (a reader made by Engine.read_zips)"""
        t, d, in_dir = _c.c_uint16(), _c.c_uint16(), _c.c_int()
        self.engine._check(self.engine.lib.zh_zip_entry_v1(self._h, i, _c.byref(t), _c.byref(d), _c.byref(in_dir)))
        return t.value, d.value, in_dir.value

    def find(self, path):
        raw = path.encode("utf-8", "surrogateescape")
        idx = _c.c_size_t()
        self.engine._check(self.engine.lib.zh_zip_find(self._h, raw, len(raw), _c.byref(idx)))
        return idx.value

    def extract_batch(self, indices):
        """-> (list of bytes | None, statuses) for the records at `indices`, one GPU batch."""
        n = len(indices)
        idx = (_c.c_size_t * n)(*indices)
        dsts = (_c.c_void_p * n)()
        lens = (_c.c_size_t * n)()
        sts = (_c.c_int32 * n)()
        rc = self.engine.lib.zh_zip_extract_batch(self.engine._h, self._h, idx, n, dsts, lens, sts)
        outs = []
        try:
            for i in range(n):
                outs.append(_c.string_at(dsts[i], lens[i]) if dsts[i] and sts[i] == 0 else None)
        finally:
            for i in range(n):
                if dsts[i]:
                    self.engine.lib.zh_free(dsts[i])
        self.engine._check(rc)
        return outs, list(sts)

    def extract_file(self, path):
        outs, sts = self.extract_batch([self.find(path)])
        self.engine._check(sts[0])
        return outs[0]

    def close(self):
        if self._h:
            self.engine.lib.zh_zip_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TarEntry(_c.Structure):
    _fields_ = [("path", _c.c_void_p), ("path_len", _c.c_size_t), ("linkname", _c.c_void_p),
                ("linkname_len", _c.c_size_t), ("typeflag", _c.c_char), ("mode", _c.c_uint32),
                ("mtime", _c.c_int64), ("offset", _c.c_uint64), ("size", _c.c_uint64)]


class TarReader:
    """zh_tar_reader: the entries of a .tar.gz / .tar image (tarballs.nim:61-124)."""

    def __init__(self, engine, image, handle=None):
        """handle: a reader zh_tar_open_batch made of `image` (Engine.open_tars); None: zh_tar_open"""
        self.engine = engine
        self._image = bytes(image)  # an uncompressed tarball stays borrowed until close
        h = _c.c_void_p()
        if handle is None:
            engine._check(engine.lib.zh_tar_open(engine._h, self._image, len(self._image), _c.byref(h)))
        else:
            h = _c.c_void_p(handle)
        self._h = h
        n = _c.c_size_t()
        base = engine.lib.zh_tar_data(h, _c.byref(n))
        self.data = _c.string_at(base, n.value) if n.value else b""
        self.entries = []
        for i in range(engine.lib.zh_tar_num_entries(h)):
            e = TarEntry()
            engine._check(engine.lib.zh_tar_entry_at(h, i, _c.byref(e)))
            self.entries.append({
                "path": _c.string_at(e.path, e.path_len), "linkname": _c.string_at(e.linkname, e.linkname_len),
                "typeflag": e.typeflag, "mode": e.mode, "mtime": e.mtime, "offset": e.offset, "size": e.size})

    def contents(self, i):
        e = self.entries[i]
        return self.data[e["offset"]:e["offset"] + e["size"]]

    def close(self):
        if self._h:
            self.engine.lib.zh_tar_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TarNewEntry(_c.Structure):
    _fields_ = [("path", _c.c_char_p), ("path_len", _c.c_size_t), ("contents", _c.c_void_p), ("len", _c.c_size_t),
                ("kind", _c.c_char), ("mtime", _c.c_int64)]


def _tar_entries(entries):
    """A Tarball's contents (tarballs_v1.nim:8-18) as (path bytes, contents bytes, kind byte, mtime) tuples: an ordered
    mapping or (path, value) pairs; a value is the contents, or (contents, kind, mtime) -- kind '0' / '5', mtime the
    Unix time (defaults '0' and 0)."""
    out = []
    for path, v in (entries.items() if hasattr(entries, "items") else entries):
        contents, kind, mtime = v, "0", 0
        if isinstance(v, tuple):
            contents, kind, mtime = v + ("0", 0)[len(v) - 1:]
        p = path.encode("utf-8", "surrogateescape") if isinstance(path, str) else bytes(path)
        k = kind.encode("latin-1") if isinstance(kind, str) else bytes(kind)
        out.append((p, bytes(contents), k if len(k) == 1 else b"\0", int(mtime)))  # (a kind of other length: rejected)
    return out


class ZipNewEntry(_c.Structure):
    _fields_ = [("path", _c.c_char_p), ("path_len", _c.c_size_t), ("contents", _c.c_void_p), ("len", _c.c_size_t),
                ("is_directory", _c.c_int), ("dos_time", _c.c_uint16), ("dos_date", _c.c_uint16)]


def _zip_entries(entries):
    """A ZipArchive's contents (ziparchives_v1.nim:12-21) as (path bytes, contents, is_directory, dos_time, dos_date)
    tuples: an ordered mapping or (path, value) pairs; a value is the contents, or (contents, is_directory, dos_time,
    dos_date) (defaults False, 0, 0).  Contents may be any buffer: bytes and writable buffers (an mmap, a bytearray) go
    to the library as they are, other read-only buffers are copied first (the library reads nothing of an entry it
    refuses before compressing)."""
    out = []
    for path, v in (entries.items() if hasattr(entries, "items") else entries):
        contents, is_dir, t, d = v, False, 0, 0
        if isinstance(v, tuple):
            contents, is_dir, t, d = v + (False, 0, 0)[len(v) - 1:]
        p = path.encode("utf-8", "surrogateescape") if isinstance(path, str) else bytes(path)
        out.append((p, contents, bool(is_dir), int(t), int(d)))
    return out


def _zip_tables(tables, dos_time, dos_date):
    """createZipArchive's tables (ziparchives.nim:455) as lists of _zip_entries tuples: ordered mappings or (path,
    contents) pairs, every entry stamped with the call's dos_time / dos_date as the reference stamps them with one
    msdos(getTime()); a value may also be (contents, dos_time, dos_date) with a pair of its own.  is_directory stays
    False: zh_zip_create_batch does not read it."""
    out = []
    for table in tables:
        group = []
        for path, v in (table.items() if hasattr(table, "items") else table):
            contents, t, d = v if isinstance(v, tuple) else (v, dos_time, dos_date)
            p = path.encode("utf-8", "surrogateescape") if isinstance(path, str) else bytes(path)
            group.append((p, contents, False, int(t), int(d)))
        out.append(group)
    return out


def _zip_table(groups):
    """The C arrays of the zip writers for lists of _zip_entries tuples (kept alive by the returned tuple)."""
    keep = []

    def fill(e, p, c, is_dir, t, d):
        addr, n, k = _buffer_address(c)
        keep.append(k)
        e.path, e.path_len, e.contents, e.len = p, len(p), addr, n
        e.is_directory, e.dos_time, e.dos_date = int(is_dir), t & 0xFFFF, d & 0xFFFF
    arr, first, n, flat = _writer_table(ZipNewEntry, groups, fill)
    return arr, first, n, (flat, keep)


def _writer_table(entry_type, groups, fill):
    """groups: lists of entry tuples -> (entry array, first[], number of groups, the entry tuples); fill(entry, *tuple)
    sets one entry"""
    flat = [e for g in groups for e in g]
    arr = (entry_type * max(1, len(flat)))()
    for i, e in enumerate(flat):
        fill(arr[i], *e)
    first = [0]
    for g in groups:
        first.append(first[-1] + len(g))
    return arr, (_c.c_size_t * len(first))(*first), len(groups), flat


def _buffer_address(obj):
    """-> (address or None, length, the object that keeps the memory alive)"""
    if not isinstance(obj, bytes):
        mv = memoryview(obj)
        if mv.readonly or not mv.contiguous:
            obj = bytes(mv)
        else:
            n = mv.nbytes
            return (_c.addressof(_c.c_char.from_buffer(mv.cast("B"))) if n else None), n, mv
    return (_c.cast(_c.c_char_p(obj), _c.c_void_p).value if obj else None), len(obj), obj


class Engine:
    def __init__(self, lib_path, device=-1, stream=None):
        self.lib = load_library(lib_path)
        h = _c.c_void_p()
        st = self.lib.zh_create(device, stream, _c.byref(h))
        if st != 0:
            raise ZippyError(st, "zh_create: %s (no usable MI355X? zippy_amd has no CPU fallback)" %
                             self.lib.zh_strerror(st).decode())
        self._h = h

    def close(self):
        if self._h:
            self.lib.zh_destroy(self._h)
            self._h = None

    def _check(self, st):
        if st != 0:
            msg = self.lib.zh_strerror(st).decode()
            if st == 20:
                msg += ": " + self.lib.zh_last_error(self._h).decode()
            raise ZippyError(st, msg)

    def set_gzip_fname_len(self, k):
        self.lib.zh_set_gzip_fname_len(self._h, k)

    def set_inflate_mode(self, mode):
        """0: parallel token decode + writer (default), 1: serial two-wave decoder, -1: default."""
        self.lib.zh_set_inflate_mode(self._h, mode)

    def set_l1_parse(self, mode):
        """BestSpeed match finder: 0 the reference's parse (byte-identical streams, default),
        1 the parallel parse (valid streams of about the same size), -1: default / ZH_L1_PARSE."""
        self.lib.zh_set_l1_parse(self._h, mode)

    def chain_links_parallel(self):
        """True: the device passed zh_create's probe and the chain levels' links are built by the class-sorted
        kernels; False: by the in-order ones (a failed probe, or ZH_CHAIN_PREV=serial)."""
        return bool(self.lib.zh_chain_links_parallel(self._h))

    def set_host_pipeline(self, min_batch_bytes=0, group_bytes=0):
        self.lib.zh_set_host_pipeline(self._h, min_batch_bytes, group_bytes)

    def compress_bound(self, n, data_format=dfGzip):
        return self.lib.zh_compress_bound(n, data_format)

    # ---- host-buffer batch API ----
    def _batch(self, fn, bufs, *mid):
        n = len(bufs)
        keep = [bytes(b) for b in bufs]
        srcs = (_c.c_void_p * n)(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in keep])
        lens = (_c.c_size_t * n)(*[len(k) for k in keep])
        dsts = (_c.c_void_p * n)()
        dlens = (_c.c_size_t * n)()
        sts = (_c.c_int32 * n)()
        rc = fn(self._h, srcs, lens, n, *mid, dsts, dlens, sts)
        outs = []
        try:
            for i in range(n):
                outs.append(_c.string_at(dsts[i], dlens[i]) if dsts[i] and sts[i] == 0 else None)
        finally:
            for i in range(n):
                if dsts[i]:
                    self.lib.zh_free(dsts[i])
        self._check(rc)
        return outs, list(sts)

    def compress_batch(self, bufs, level=DefaultCompression, data_format=dfGzip):
        """-> (list of bytes | None, list of statuses)"""
        return self._batch(self.lib.zh_compress_batch, bufs, level, data_format)

    def uncompress_batch(self, bufs, data_format=dfDetect):
        return self._batch(self.lib.zh_uncompress_batch, bufs, data_format)

    def compress_batch_crc32(self, bufs, level=DefaultCompression, data_format=dfGzip):
        """compress_batch that also returns crc32(bufs[i]) (zh_compress_batch_crc32) -> (outs, statuses, crcs)"""
        crcs = (_c.c_uint32 * max(1, len(bufs)))()
        outs, sts = self._batch(lambda *a: self.lib.zh_compress_batch_crc32(*a, crcs), bufs, level, data_format)
        return outs, sts, list(crcs)[:len(bufs)]

    def uncompress_batch_sized(self, bufs, data_format=dfDetect, size_hints=None, want_crcs=True):
        """uncompress_batch with the output sizes known up front (zh_uncompress_batch_sized): size_hints[i] replaces
        the guess for streams without a size field (None: no hints).  -> (outs, statuses, crcs); crcs[i] is the
        CRC-32 of output i where its status is 0 (None without want_crcs)."""
        n = len(bufs)
        hints = _u64(size_hints) if size_hints is not None else None
        if hints is not None and len(hints) != n:
            raise ValueError("size_hints: one per buffer")
        crcs = (_c.c_uint32 * max(1, n))() if want_crcs else None
        outs, sts = self._batch(lambda *a: self.lib.zh_uncompress_batch_sized(*a, crcs), bufs, data_format, hints)
        return outs, sts, (list(crcs)[:n] if want_crcs else None)

    def _batch_into(self, fn, bufs, outs, *mid):
        """`outs`: writable buffers (bytearray / ctypes arrays) the library fills.
        -> (lengths, statuses): lengths[i] is the result's size, also when it did not fit."""
        n = len(bufs)
        keep = [bytes(b) if not isinstance(b, bytes) else b for b in bufs]
        srcs = (_c.c_void_p * n)(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in keep])
        lens = (_c.c_size_t * n)(*[len(k) for k in keep])
        views = [(_c.c_char * len(o)).from_buffer(o) if len(o) else None for o in outs]
        dsts = (_c.c_void_p * n)(*[_c.addressof(v) if v is not None else None for v in views])
        caps = (_c.c_size_t * n)(*[len(o) for o in outs])
        dlens, sts = (_c.c_size_t * n)(), (_c.c_int32 * n)()
        self._check(fn(self._h, srcs, lens, n, *mid, dsts, caps, dlens, sts))
        filled = [dsts[i] is not None or dlens[i] == 0 for i in range(n)]
        return list(dlens), list(sts), filled

    def compress_batch_into(self, bufs, outs, level=DefaultCompression, data_format=dfGzip):
        return self._batch_into(self.lib.zh_compress_batch_into, bufs, outs, level, data_format)

    def uncompress_batch_into(self, bufs, outs, data_format=dfDetect):
        return self._batch_into(self.lib.zh_uncompress_batch_into, bufs, outs, data_format)

    def _raise_first(self, outs, sts):
        for st in sts:
            if st != 0:
                raise ZippyError(st, self.lib.zh_strerror(st).decode())
        return outs

    def compress(self, src, level=DefaultCompression, data_format=dfGzip):
        try:
            outs, sts = self.compress_batch([src], level, data_format)
        except ZippyError:
            raise
        return self._raise_first(outs, sts)[0]

    def uncompress(self, src, data_format=dfDetect):
        outs, sts = self.uncompress_batch([src], data_format)
        return self._raise_first(outs, sts)[0]

    def segment_stats(self):
        """(streams cut into segments, streams whose chain of segments held) since the context was made."""
        cut, held = _c.c_uint64(), _c.c_uint64()
        self._check(self.lib.zh_debug_segment_stats(self._h, _c.byref(cut), _c.byref(held)))
        return cut.value, held.value

    def debug_huffman(self, freq, min_codes, limit, contract=False):
        """One prefix code from a histogram, by the byte-identical builder or by contract mode's
        (zh_debug_huffman) -> (codes, lens) as numpy arrays of numCodes entries."""
        import numpy as np
        f = np.ascontiguousarray(freq, dtype=np.uint32)
        codes = (_c.c_uint16 * (len(f) + 2))()
        lens = (_c.c_uint8 * (len(f) + 2))()
        n = _c.c_int()
        self._check(self.lib.zh_debug_huffman(self._h, f.ctypes.data_as(_c.POINTER(_c.c_uint32)), len(f), min_codes, limit,
                                              1 if contract else 0, codes, lens, _c.byref(n)))
        return np.array(codes[:n.value], dtype=np.uint16), np.array(lens[:n.value], dtype=np.uint8)

    # ---- ZIP archives (ziparchives.nim) ----
    def open_zip(self, image):
        return ZipReader(self, image)

    def open_zips(self, images):
        """zh_zip_open_all_batch: many archives opened and extracted in one call -> (readers, statuses); readers[t]
        is a ZipReader with .data / .entry_status(i) / .contents(i), or None where the archive did not open."""
        return self._open_zips(self.lib.zh_zip_open_all_batch, images)

    def read_zips(self, images):
        """zh_zip_read_batch: ZipArchive.open (ziparchives_v1.nim:105-349) of every image in one call -> (readers,
        statuses); readers[t] is a ZipReader with .data / .contents(i) / .entry_v1(i), or None unless statuses[t] is 0."""
        return self._open_zips(self.lib.zh_zip_read_batch, images)

    def _open_zips(self, fn, images):
        images = [bytes(b) for b in images]
        n = len(images)
        srcs = (_c.c_void_p * n)(*[_c.cast(_c.c_char_p(b), _c.c_void_p) if b else None for b in images])
        lens = (_c.c_size_t * n)(*[len(b) for b in images])
        handles, sts = (_c.c_void_p * n)(), (_c.c_int32 * n)()
        self._check(fn(self._h, srcs, lens, n, handles, sts))
        return [ZipReader(self, b, h) if h else None for b, h in zip(images, handles)], list(sts)

    def create_zip(self, entries, dos_time=0, dos_date=0):
        """entries: ordered (path, contents) pairs -> archive bytes (createZipArchive)."""
        entries = list(entries.items()) if hasattr(entries, "items") else list(entries)
        n = len(entries)
        names = [p.encode("utf-8", "surrogateescape") if isinstance(p, str) else bytes(p) for p, _ in entries]
        blobs = [bytes(c) for _, c in entries]
        c_names = (_c.c_char_p * n)(*names)
        c_nlens = (_c.c_size_t * n)(*[len(x) for x in names])
        c_blobs = (_c.c_void_p * n)(*[_c.cast(_c.c_char_p(b), _c.c_void_p) for b in blobs])
        c_blens = (_c.c_size_t * n)(*[len(b) for b in blobs])
        dst, dlen = _c.c_void_p(), _c.c_size_t()
        self._check(self.lib.zh_zip_create(self._h, c_names, c_nlens, c_blobs, c_blens, n, dos_time, dos_date,
                                           _c.byref(dst), _c.byref(dlen)))
        try:
            return _c.string_at(dst, dlen.value)
        finally:
            self.lib.zh_free(dst)

    def open_tar(self, image):
        return TarReader(self, image)

    def open_tars(self, images):
        """zh_tar_open_batch: the images of many .tar.gz / .tar files opened in one call -> (readers, statuses);
        readers[t] is a TarReader, or None where statuses[t] != 0."""
        images = [bytes(b) for b in images]
        n = len(images)
        srcs = (_c.c_void_p * n)(*[_c.cast(_c.c_char_p(b), _c.c_void_p) if b else None for b in images])
        lens = (_c.c_size_t * n)(*[len(b) for b in images])
        handles, sts = (_c.c_void_p * n)(), (_c.c_int32 * n)()
        self._check(self.lib.zh_tar_open_batch(self._h, srcs, lens, n, handles, sts))
        return [TarReader(self, b, h) if h else None for b, h in zip(images, handles)], list(sts)

    def read_tars(self, images, formats=None):
        """zh_tar_read_batch: Tarball.open (tarballs_v1.nim:66-157) of every image in one call -> (readers, statuses);
        formats: tfDetect / tfUncompressed / tfGzip (0 / 1 / 2), one an image, None: all detect.  readers[t] is a TarReader
        whose entries are the table's keys in the table's order, or None where statuses[t] != 0."""
        images = [bytes(b) for b in images]
        n = len(images)
        srcs = (_c.c_void_p * n)(*[_c.cast(_c.c_char_p(b), _c.c_void_p) if b else None for b in images])
        lens = (_c.c_size_t * n)(*[len(b) for b in images])
        if formats is not None and len(formats) != n:
            raise ValueError("formats: one value an image")
        fmts = None if formats is None else (_c.c_int32 * n)(*[int(f) for f in formats])
        handles, sts = (_c.c_void_p * n)(), (_c.c_int32 * n)()
        self._check(self.lib.zh_tar_read_batch(self._h, srcs, lens, fmts, n, handles, sts))
        return [TarReader(self, b, h) if h else None for b, h in zip(images, handles)], list(sts)

    def create_tars(self, tarballs, data_format=dfGzip, level=DefaultCompression):
        """writeTarball (tarballs_v1.nim:203-270) of every tarball in one call (zh_tar_create_batch).
        tarballs: a list of entry collections (see _tar_entries); data_format: dfGzip or TAR_PLAIN.
        -> (list of bytes | None, statuses)"""
        return self.create_tars_prepared(self.prepare_tars(tarballs), data_format, level)

    @staticmethod
    def prepare_tars(tarballs):
        """The C arrays of zh_tar_create_batch for `tarballs` (kept alive by the returned tuple)."""
        def fill(e, p, c, k, m):
            e.path, e.path_len = p, len(p)
            e.contents = _c.cast(_c.c_char_p(c), _c.c_void_p) if c else None
            e.len, e.kind, e.mtime = len(c), k, m
        return _writer_table(TarNewEntry, [_tar_entries(t) for t in tarballs], fill)

    def create_tars_prepared(self, prepared, data_format=dfGzip, level=DefaultCompression):
        return self._run_writer(self.lib.zh_tar_create_batch, prepared, data_format, level)

    def create_tar(self, entries, data_format=dfGzip, level=DefaultCompression):
        """One tarball's bytes; raises ZippyError on failure."""
        outs, sts = self.create_tars([entries], data_format, level)
        return self._raise_first(outs, sts)[0]

    def write_zips(self, archives, level=DefaultCompression):
        """writeZipArchive (ziparchives_v1.nim:371-486) of every archive in one call (zh_zip_write_batch).
        archives: a list of entry collections (see _zip_entries).  -> (list of bytes | None, statuses)"""
        return self.write_zips_prepared(self.prepare_zips(archives), level)

    @staticmethod
    def prepare_zips(archives):
        """The C arrays of zh_zip_write_batch for `archives` (kept alive by the returned tuple)."""
        return _zip_table([_zip_entries(a) for a in archives])

    def write_zips_prepared(self, prepared, level=DefaultCompression):
        return self._run_writer(self.lib.zh_zip_write_batch, prepared, level)

    def _run_writer(self, fn, prepared, *args):
        """fn(ctx, entries, first, n, *args, dsts, dst_lens, statuses) of a batch writer -> (list of bytes | None, statuses)"""
        arr, c_first, n, _ = prepared
        dsts, dlens, sts = (_c.c_void_p * max(1, n))(), (_c.c_size_t * max(1, n))(), (_c.c_int32 * max(1, n))()
        rc = fn(self._h, arr, c_first, n, *args, dsts, dlens, sts)
        outs = []
        try:
            for t in range(n):
                outs.append(_c.string_at(dsts[t], dlens[t]) if dsts[t] and sts[t] == 0 else None)
        finally:
            for t in range(n):
                if dsts[t]:
                    self.lib.zh_free(dsts[t])
        self._check(rc)
        return outs, list(sts)[:n]

    def write_zip(self, entries, level=DefaultCompression):
        """One archive's bytes; raises ZippyError on failure."""
        outs, sts = self.write_zips([entries], level)
        return self._raise_first(outs, sts)[0]

    def create_zips(self, tables, dos_time=0, dos_date=0, level=BestSpeed):
        """createZipArchive (ziparchives.nim:455-634) of every table in one call (zh_zip_create_batch).
        tables: a list of ordered mappings / (path, contents) pairs (see _zip_tables); BestSpeed is the reference's
        level.  -> (list of bytes | None, statuses)"""
        return self.create_zips_prepared(self.prepare_zips_v2(tables, dos_time, dos_date), level)

    @staticmethod
    def prepare_zips_v2(tables, dos_time=0, dos_date=0):
        """The C arrays of zh_zip_create_batch for `tables` (kept alive by the returned tuple)."""
        return _zip_table(_zip_tables(tables, dos_time, dos_date))

    def create_zips_prepared(self, prepared, level=BestSpeed):
        return self._run_writer(self.lib.zh_zip_create_batch, prepared, level)

    def create_zips_one(self, entries, dos_time=0, dos_date=0, level=BestSpeed):
        """One archive's bytes through the batch call; raises ZippyError on failure."""
        outs, sts = self.create_zips([entries], dos_time, dos_date, level)
        return self._raise_first(outs, sts)[0]

    def crc32_batch(self, bufs):
        n = len(bufs)
        keep = [bytes(b) for b in bufs]
        srcs = (_c.c_void_p * n)(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in keep])
        lens = (_c.c_size_t * n)(*[len(k) for k in keep])
        out = (_c.c_uint32 * n)()
        self._check(self.lib.zh_crc32_batch(self._h, srcs, lens, n, out))
        return list(out)

    # ---- block-parallel form of one large buffer (BASELINE config 5) ----
    def compress_blocks(self, src, level=DefaultCompression, data_format=dfGzip, block_bytes=32768):
        """-> (compressed bytes, [(bit_off, out_off), ...])"""
        src = bytes(src)
        dst, dlen = _c.c_void_p(), _c.c_size_t()
        idx, n = _c.POINTER(_c.c_uint64)(), _c.c_size_t()
        self._check(self.lib.zh_compress_blocks(self._h, src, len(src), level, data_format, block_bytes,
                                                _c.byref(dst), _c.byref(dlen), _c.byref(idx), _c.byref(n)))
        try:
            return _c.string_at(dst, dlen.value), [(idx[2 * i], idx[2 * i + 1]) for i in range(n.value)]
        finally:
            self.lib.zh_free(dst)
            self.lib.zh_free(idx)

    def uncompress_indexed(self, src, index, data_format=dfDetect):
        src = bytes(src)
        flat = _u64([v for e in index for v in e])
        dst, dlen = _c.c_void_p(), _c.c_size_t()
        self._check(self.lib.zh_uncompress_indexed(self._h, src, len(src), data_format, flat, len(index),
                                                   _c.byref(dst), _c.byref(dlen)))
        try:
            return _c.string_at(dst, dlen.value)
        finally:
            self.lib.zh_free(dst)

    # ---- byte ranges of block-indexed streams ----
    @staticmethod
    def _range_tables(indexes, ranges):
        """The C arrays both ranges calls share: every stream's index back to back with first[], the ranges as three
        parallel uint64 arrays (values wrap at 2^64 like the C types)."""
        flat = _u64([v for idx in indexes for e in idx for v in e])
        first = [0]
        for idx in indexes:
            first.append(first[-1] + len(idx))
        m64 = (1 << 64) - 1
        cols = [_u64([int(r[k]) & m64 for r in ranges]) for k in range(3)]
        return flat, (_c.c_size_t * len(first))(*first), cols

    def uncompress_ranges(self, streams, indexes, ranges):
        """Bytes [off, off + len) of the uncompressed data of streams[stream] for every (stream, off, len) of `ranges`,
        one call (zh_uncompress_ranges); indexes[s]: stream s's [(bit_off, out_off), ...] as compress_blocks returns it.
        -> (list of bytes | None, statuses)"""
        if len(indexes) != len(streams):
            raise ValueError("indexes: one per stream")
        ns, nr = len(streams), len(ranges)
        keep = [bytes(b) for b in streams]
        srcs = (_c.c_void_p * max(1, ns))(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in keep])
        lens = (_c.c_size_t * max(1, ns))(*[len(k) for k in keep])
        flat, first, (rs, ro, rl) = self._range_tables(indexes, ranges)
        dsts, dlens, sts = (_c.c_void_p * max(1, nr))(), (_c.c_size_t * max(1, nr))(), (_c.c_int32 * max(1, nr))()
        rc = self.lib.zh_uncompress_ranges(self._h, srcs, lens, ns, flat, first, nr, rs, ro, rl, dsts, dlens, sts)
        outs = []
        try:
            for r in range(nr):
                outs.append(_c.string_at(dsts[r], dlens[r]) if dsts[r] and sts[r] == 0 else None)
        finally:
            for r in range(nr):
                if dsts[r]:
                    self.lib.zh_free(dsts[r])
        self._check(rc)
        return outs, list(sts)[:nr]

    def plan_uncompress_ranges(self, src_off, src_len, indexes, ranges, dst_off, dst_cap):
        """zh_plan_uncompress_ranges: streams d_src[src_off[s] .. + src_len[s]) with indexes[s], ranges as in
        uncompress_ranges, slots d_dst[dst_off[r] .. + dst_cap[r]) -> a Plan of len(ranges)."""
        if len(indexes) != len(src_off):
            raise ValueError("indexes: one per stream")
        h = _c.c_void_p()
        flat, first, (rs, ro, rl) = self._range_tables(indexes, ranges)
        self._check(self.lib.zh_plan_uncompress_ranges(self._h, len(src_off), _u64(src_off), _u64(src_len), flat, first,
                                                       len(ranges), rs, ro, rl, _u64(dst_off), _u64(dst_cap),
                                                       _c.byref(h)))
        return Plan(self, h, len(ranges))

    def debug_range_stats(self):
        """(uploaded bytes, blocks decoded in place, blocks decoded via scratch) of the last ranges call / plan run."""
        up, ip, sc = _c.c_uint64(), _c.c_uint64(), _c.c_uint64()
        self._check(self.lib.zh_debug_range_stats(self._h, _c.byref(up), _c.byref(ip), _c.byref(sc)))
        return up.value, ip.value, sc.value

    # ---- BGZF (blocked gzip) ----
    def bgzf_compress_batch(self, bufs, level=DefaultCompression, block_bytes=0):
        """One BGZF file per buffer (zh_bgzf_write_batch): members of block_bytes (0: 65280) and the EOF marker.
        -> (list of bytes | None, statuses)"""
        return self._batch(self.lib.zh_bgzf_write_batch, bufs, level, block_bytes)

    def bgzf_uncompress_batch(self, images, want_eof=False):
        """The uncompressed data of BGZF files (zh_bgzf_read_batch) -> (list of bytes | None, statuses), with
        want_eof also the list of has_eof flags."""
        eof = (_c.c_uint8 * max(1, len(images)))()
        outs, sts = self._batch(lambda *a: self.lib.zh_bgzf_read_batch(*a, eof), images)
        return (outs, sts, list(eof)[:len(images)]) if want_eof else (outs, sts)

    def bgzf_index_batch(self, images):
        """The members of BGZF files from their headers alone (zh_bgzf_index_batch) -> (indexes, statuses, has_eof);
        indexes[i]: [(coff, uoff), ...] closed by (end of the walk, total), None where the image failed."""
        n = len(images)
        keep = [bytes(b) for b in images]
        srcs = (_c.c_void_p * max(1, n))(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in keep])
        lens = (_c.c_size_t * max(1, n))(*[len(k) for k in keep])
        idx, first = _c.POINTER(_c.c_uint64)(), (_c.c_size_t * (n + 1))()
        sts, eof = (_c.c_int32 * max(1, n))(), (_c.c_uint8 * max(1, n))()
        rc = self.lib.zh_bgzf_index_batch(self._h, srcs, lens, n, _c.byref(idx), first, sts, eof)
        try:
            self._check(rc)
            out = [[(idx[2 * k], idx[2 * k + 1]) for k in range(first[i], first[i + 1])] if sts[i] == 0 else None
                   for i in range(n)]
        finally:
            if idx:
                self.lib.zh_free(idx)
        return out, list(sts)[:n], list(eof)[:n]

    def bgzf_read_ranges(self, images, indexes, ranges):
        """Bytes [off, off + len) of the uncompressed data of images[image] for every (image, off, len) of `ranges`, one
        call (zh_bgzf_read_ranges); indexes[i]: image i's [(coff, uoff), ...] as bgzf_index_batch returns it (None, what
        it returns for an image that failed, is an index of no entries: that image's ranges fail with status 13).
        -> (list of bytes | None, statuses)"""
        if len(indexes) != len(images):
            raise ValueError("indexes: one per image")
        indexes = [idx if idx is not None else [] for idx in indexes]
        ns, nr = len(images), len(ranges)
        keep = [bytes(b) for b in images]
        srcs = (_c.c_void_p * max(1, ns))(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in keep])
        lens = (_c.c_size_t * max(1, ns))(*[len(k) for k in keep])
        flat, first, (rs, ro, rl) = self._range_tables(indexes, ranges)
        dsts, dlens, sts = (_c.c_void_p * max(1, nr))(), (_c.c_size_t * max(1, nr))(), (_c.c_int32 * max(1, nr))()
        rc = self.lib.zh_bgzf_read_ranges(self._h, srcs, lens, ns, flat, first, nr, rs, ro, rl, dsts, dlens, sts)
        outs = []
        try:
            for r in range(nr):
                outs.append(_c.string_at(dsts[r], dlens[r]) if dsts[r] and sts[r] == 0 else None)
        finally:
            for r in range(nr):
                if dsts[r]:
                    self.lib.zh_free(dsts[r])
        self._check(rc)
        return outs, list(sts)[:nr]

    # ---- any gzip file: several members, FEXTRA / FNAME / FCOMMENT / FHCRC ----
    def gzip_read_batch(self, images, want_data=True, want_members=True):
        """The uncompressed data and the members of gzip files of any shape (zh_gzip_read_batch) -> (list of bytes |
        None, statuses, members); members[i]: image i's list of dicts with zh_gzip_member's fields, None where the
        image failed.  want_data=False: every member is still decoded and verified, no data comes down (outputs are
        None); want_members=False: members is None."""
        n = len(images)
        keep = [bytes(b) for b in images]
        srcs = (_c.c_void_p * max(1, n))(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in keep])
        lens = (_c.c_size_t * max(1, n))(*[len(k) for k in keep])
        dsts = (_c.c_void_p * max(1, n))() if want_data else None
        dlens = (_c.c_size_t * max(1, n))() if want_data else None
        sts = (_c.c_int32 * max(1, n))()
        mem = _c.c_void_p() if want_members else None
        first = (_c.c_size_t * (n + 1))() if want_members else None
        rc = self.lib.zh_gzip_read_batch(self._h, srcs, lens, n, dsts, dlens, sts, _c.byref(mem) if want_members else None,
                                         first)
        outs, members = [None] * n, None
        try:
            for i in range(n):
                if want_data and dsts[i] and sts[i] == 0:
                    outs[i] = _c.string_at(dsts[i], dlens[i])
            if want_members and rc == 0:
                arr = _c.cast(mem, _c.POINTER(GzipMember))
                members = [[arr[k].as_dict() for k in range(first[i], first[i + 1])] if sts[i] == 0 else None
                           for i in range(n)]
        finally:
            for i in range(n):
                if want_data and dsts[i]:
                    self.lib.zh_free(dsts[i])
            if want_members and mem:
                self.lib.zh_free(mem)
        self._check(rc)
        return outs, list(sts)[:n], members

    def debug_gzip_stats(self):
        """(candidates, input bytes the budgeted sizing pass consumed, frontier rounds) of the last gzip_read_batch."""
        c, b, r = _c.c_uint64(), _c.c_uint64(), _c.c_uint64()
        self._check(self.lib.zh_debug_gzip_stats(self._h, _c.byref(c), _c.byref(b), _c.byref(r)))
        return c.value, b.value, r.value

    # ---- seek indexes for foreign deflate streams ----
    def seek_index_batch(self, srcs, dataFormat=dfDetect, span=0, want_data=False):
        """One seek index (a blob of bytes, include/zippy_hip.h) per stream (zh_seek_index_batch); span: uncompressed
        bytes between points (0: 1 MiB).  -> (indexes, statuses), with want_data (indexes, statuses, outputs); an index
        and an output are None where the stream's status is not 0."""
        n = len(srcs)
        keep = [bytes(b) for b in srcs]
        ptrs = (_c.c_void_p * max(1, n))(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in keep])
        lens = (_c.c_size_t * max(1, n))(*[len(k) for k in keep])
        idx, ilens, sts = (_c.c_void_p * max(1, n))(), (_c.c_size_t * max(1, n))(), (_c.c_int32 * max(1, n))()
        dsts, dlens = ((_c.c_void_p * max(1, n))(), (_c.c_size_t * max(1, n))()) if want_data else (None, None)
        rc = self.lib.zh_seek_index_batch(self._h, ptrs, lens, n, int(dataFormat), int(span), idx, ilens, dsts, dlens, sts)
        blobs, outs = [], []
        try:
            for i in range(n):
                blobs.append(_c.string_at(idx[i], ilens[i]) if idx[i] and sts[i] == 0 else None)
                if want_data:
                    outs.append(_c.string_at(dsts[i], dlens[i]) if dsts[i] and sts[i] == 0 else None)
        finally:
            for i in range(n):
                if idx[i]:
                    self.lib.zh_free(idx[i])
                if want_data and dsts[i]:
                    self.lib.zh_free(dsts[i])
        self._check(rc)
        return (blobs, list(sts)[:n], outs) if want_data else (blobs, list(sts)[:n])

    def seek_read_ranges(self, streams, indexes, ranges):
        """Bytes [off, off + len) of the uncompressed data of streams[stream] for every (stream, off, len) of `ranges`,
        one call (zh_seek_read_ranges); indexes[s]: stream s's blob as seek_index_batch returns it (None, what it
        returns for a stream that failed, is a blob of no bytes: that stream's ranges fail with status 13).
        -> (list of bytes | None, statuses)"""
        if len(indexes) != len(streams):
            raise ValueError("indexes: one per stream")
        ns, nr = len(streams), len(ranges)
        keep = [bytes(b) for b in streams]
        blobs = [bytes(b) if b is not None else b"" for b in indexes]
        srcs = (_c.c_void_p * max(1, ns))(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in keep])
        lens = (_c.c_size_t * max(1, ns))(*[len(k) for k in keep])
        idx = (_c.c_void_p * max(1, ns))(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in blobs])
        ilens = (_c.c_size_t * max(1, ns))(*[len(k) for k in blobs])
        m64 = (1 << 64) - 1
        rs, ro, rl = [_u64([int(r[k]) & m64 for r in ranges]) for k in range(3)]
        dsts, dlens, sts = (_c.c_void_p * max(1, nr))(), (_c.c_size_t * max(1, nr))(), (_c.c_int32 * max(1, nr))()
        rc = self.lib.zh_seek_read_ranges(self._h, srcs, lens, ns, idx, ilens, nr, rs, ro, rl, dsts, dlens, sts)
        outs = []
        try:
            for r in range(nr):
                outs.append(_c.string_at(dsts[r], dlens[r]) if dsts[r] and sts[r] == 0 else None)
        finally:
            for r in range(nr):
                if dsts[r]:
                    self.lib.zh_free(dsts[r])
        self._check(rc)
        return outs, list(sts)[:nr]

    # ---- resumable uncompress ----
    def uncompress_resume_batch(self, srcs, states=None, max_out=1 << 20, last=None, dataFormat=dfDetect):
        """One step of every stream (zh_uncompress_resume_batch): srcs[i] is the unconsumed tail of stream i followed by
        what arrived since, states[i] the state the step before returned (None: a new stream; states None: all new),
        max_out a number or one a stream, last None or one flag a stream.
        -> (outputs, consumed, new_states, why, statuses); an output is b"" and a state None where nothing came."""
        n = len(srcs)
        m = max(1, n)
        keep = [bytes(b) for b in srcs]
        blobs = [bytes(b) if b is not None else None for b in (states if states is not None else [None] * n)]
        if len(blobs) != n:
            raise ValueError("states: one per stream")
        budgets = list(max_out) if hasattr(max_out, "__len__") else [max_out] * n
        flags = [1 if f else 0 for f in last] if last is not None else None
        if len(budgets) != n or (flags is not None and len(flags) != n):
            raise ValueError("max_out, last: one per stream")
        ptrs = (_c.c_void_p * m)(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in keep])
        lens = (_c.c_size_t * m)(*[len(k) for k in keep])
        sp = (_c.c_void_p * m)(*[_c.cast(_c.c_char_p(b), _c.c_void_p) if b is not None else None for b in blobs])
        sl = (_c.c_size_t * m)(*[len(b) if b is not None else 0 for b in blobs])
        mo = _u64(budgets + [0] * (m - n))
        lf = (_c.c_uint8 * m)(*flags) if flags is not None else None
        dsts, dlens, used = (_c.c_void_p * m)(), (_c.c_size_t * m)(), (_c.c_size_t * m)()
        ns, nsl, why, sts = (_c.c_void_p * m)(), (_c.c_size_t * m)(), (_c.c_int32 * m)(), (_c.c_int32 * m)()
        rc = self.lib.zh_uncompress_resume_batch(self._h, ptrs, lens, n, int(dataFormat),
                                                 sp if states is not None else None, sl if states is not None else None,
                                                 mo, lf, dsts, dlens, used, ns, nsl, why, sts)
        outs, new_states = [], []
        try:
            for i in range(n):
                outs.append(_c.string_at(dsts[i], dlens[i]) if dsts[i] else b"")
                new_states.append(_c.string_at(ns[i], nsl[i]) if ns[i] else None)
        finally:
            for i in range(n):
                if dsts[i]:
                    self.lib.zh_free(dsts[i])
                if ns[i]:
                    self.lib.zh_free(ns[i])
        self._check(rc)
        return outs, list(used)[:n], new_states, list(why)[:n], list(sts)[:n]

    # ---- streaming compress ----
    def compress_stream_batch(self, srcs, states=None, flush=None, level=DefaultCompression, dataFormat=dfGzip,
                              block_bytes=0):
        """One step of every stream (zh_compress_stream_batch): srcs[i] is the next piece of stream i, states[i] the state
        the step before returned (None: a new stream; states None: all new), flush None (all FLUSH_SYNC), one number, or
        one FLUSH_* a stream.  level, dataFormat and block_bytes (0: 4 MiB) are those of new streams; a resumed stream
        keeps its own.
        -> (outputs, new_states, statuses); an output is b"" and a state None where nothing came."""
        n = len(srcs)
        m = max(1, n)
        keep = [bytes(b) for b in srcs]
        blobs = [bytes(b) if b is not None else None for b in (states if states is not None else [None] * n)]
        if len(blobs) != n:
            raise ValueError("states: one per stream")
        modes = None if flush is None else list(flush) if hasattr(flush, "__len__") else [flush] * n
        if modes is not None and len(modes) != n:
            raise ValueError("flush: one per stream")
        ptrs = (_c.c_void_p * m)(*[_c.cast(_c.c_char_p(k), _c.c_void_p) for k in keep])
        lens = (_c.c_size_t * m)(*[len(k) for k in keep])
        sp = (_c.c_void_p * m)(*[_c.cast(_c.c_char_p(b), _c.c_void_p) if b is not None else None for b in blobs])
        sl = (_c.c_size_t * m)(*[len(b) if b is not None else 0 for b in blobs])
        fl = (_c.c_uint8 * m)(*[int(f) & 0xff for f in modes]) if modes is not None else None
        dsts, dlens = (_c.c_void_p * m)(), (_c.c_size_t * m)()
        ns, nsl, sts = (_c.c_void_p * m)(), (_c.c_size_t * m)(), (_c.c_int32 * m)()
        rc = self.lib.zh_compress_stream_batch(self._h, ptrs, lens, n, int(level), int(dataFormat), int(block_bytes),
                                               sp if states is not None else None, sl if states is not None else None,
                                               fl, dsts, dlens, ns, nsl, sts)
        outs, new_states = [], []
        try:
            for i in range(n):
                outs.append(_c.string_at(dsts[i], dlens[i]) if dsts[i] else b"")
                new_states.append(_c.string_at(ns[i], nsl[i]) if ns[i] else None)
        finally:
            for i in range(n):
                if dsts[i]:
                    self.lib.zh_free(dsts[i])
                if ns[i]:
                    self.lib.zh_free(ns[i])
        self._check(rc)
        return outs, new_states, list(sts)[:n]

    def crc32(self, src):
        src = bytes(src)
        out = _c.c_uint32()
        self._check(self.lib.zh_crc32(self._h, src, len(src), _c.byref(out)))
        return out.value

    def adler32(self, src):
        src = bytes(src)
        out = _c.c_uint32()
        self._check(self.lib.zh_adler32(self._h, src, len(src), _c.byref(out)))
        return out.value

    # ---- device-resident API ----
    def plan_compress(self, src_off, src_len, dst_off, dst_cap, level, data_format):
        h = _c.c_void_p()
        n = len(src_off)
        self._check(self.lib.zh_plan_compress(self._h, n, _u64(src_off), _u64(src_len),
                                              _u64(dst_off), _u64(dst_cap), level, data_format,
                                              _c.byref(h)))
        return Plan(self, h, n)

    def plan_uncompress(self, src_off, src_len, dst_off, dst_cap, data_format=dfDetect):
        h = _c.c_void_p()
        n = len(src_off)
        self._check(self.lib.zh_plan_uncompress(self._h, n, _u64(src_off), _u64(src_len),
                                                _u64(dst_off), _u64(dst_cap), data_format,
                                                _c.byref(h)))
        return Plan(self, h, n)

    def plan_compress_blocks(self, src_off, src_len, dst_off, dst_cap, level, data_format, block_bytes):
        h = _c.c_void_p()
        n = len(src_off)
        self._check(self.lib.zh_plan_compress_blocks(self._h, n, _u64(src_off), _u64(src_len),
                                                     _u64(dst_off), _u64(dst_cap), level, data_format,
                                                     block_bytes, _c.byref(h)))
        return Plan(self, h, n)

    def plan_uncompress_indexed(self, src_off, src_len, dst_off, dst_cap, index, data_format=dfDetect):
        h = _c.c_void_p()
        flat = _u64([v for e in index for v in e])
        self._check(self.lib.zh_plan_uncompress_indexed(self._h, src_off, src_len, dst_off, dst_cap,
                                                        data_format, flat, len(index), _c.byref(h)))
        return Plan(self, h, 1)

    def stream(self):
        return self.lib.zh_stream(self._h)

    # ---- parity introspection ----
    def debug_tokens(self, src, level):
        import numpy as np
        src = bytes(src)
        toks = _c.POINTER(_c.c_uint16)()
        n = _c.c_size_t()
        self._check(self.lib.zh_debug_tokens(self._h, src, len(src), level, _c.byref(toks),
                                             _c.byref(n)))
        try:
            return np.ctypeslib.as_array(toks, shape=(n.value,)).copy() if n.value else np.zeros(
                0, np.uint16)
        finally:
            self.lib.zh_free(toks)
