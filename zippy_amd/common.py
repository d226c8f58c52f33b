"""src/zippy/common.nim:1-12 restated: error type, data formats, level names."""


class ZippyError(Exception):
    """Raised if an operation fails (common.nim:2).  `status` is the C-ABI
    status code (include/zippy_hip.h)."""

    def __init__(self, status, msg):
        super().__init__(msg)
        self.status = status


# CompressedDataFormat (common.nim:4-5), ordinals 0..3
dfDetect, dfZlib, dfGzip, dfDeflate = 0, 1, 2, 3

# common.nim:7-12
NoCompression = 0
BestSpeed = 1
BestCompression = 9
DefaultCompression = -1
HuffmanOnly = -2

# zh_tar_create_batch's data format for a plain .tar image (include/zippy_hip.h ZH_TAR_PLAIN)
TAR_PLAIN = -1

# TarballFormat (tarballs_v1.nim:18-19), ordinals 0..2: zh_tar_read_batch's formats
tfDetect, tfUncompressed, tfGzip = 0, 1, 2


def to_msdos(unix_time):
    """toMsDos (ziparchives_v1.nim:356-369) of a Unix time, in local time -> (dos_time, dos_date)"""
    import time
    t = time.localtime(unix_time)
    dos_time = (t.tm_sec // 2) | (t.tm_min << 5) | (t.tm_hour << 11)
    dos_date = t.tm_mday | (t.tm_mon << 5) | (((max(0, t.tm_year - 1980) & 0xFFFF) << 9) & 0xFFFF)
    return dos_time & 0xFFFF, dos_date
