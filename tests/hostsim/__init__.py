"""TEST INFRASTRUCTURE: g++ builds of the templated kernel algorithms (host runtime, single thread) used by the CPU test
suite to check hand-written gradients and the optimiser's control flow without a GPU.  The product never loads these."""
import ctypes
import os
import subprocess
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
_CACHE = {}


def build(name, extra_flags=()):
    """Compiles tests/hostsim/<name>.cpp with g++ into a temp .so and loads it."""
    key = (name, tuple(extra_flags))
    if key in _CACHE:
        return _CACHE[key]
    # builds with extra flags (development probes) get a file of their own: they must never be picked up by the test-suite
    tag = '' if not extra_flags else '_%08x' % (zlib.crc32(' '.join(extra_flags).encode()) & 0xffffffff)
    src = os.path.join(HERE, name + '.cpp')
    deps = [src] + sorted(os.path.join(HERE, '..', '..', 'glamr_amd', 'csrc', f) for f in os.listdir(os.path.join(HERE, '..', '..', 'glamr_amd', 'csrc')) if f.endswith('.hpp'))
    # the file name carries a digest of the sources: a library left in the temp directory by another checkout of this repository (whose files may
    # well be OLDER than that library) is never taken for this one's
    digest = 0
    for d in deps:
        with open(d, 'rb') as f:
            digest = zlib.crc32(f.read(), digest)
    out = os.path.join(tempfile.gettempdir(), 'glamr_hostsim_%s%s_%08x_%d.so' % (name, tag, digest & 0xffffffff, os.getuid()))
    if not os.path.exists(out):
        tmp = '%s.%d.tmp' % (out, os.getpid())
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-ffp-contract=off', src, '-o', tmp] + list(extra_flags))
        os.replace(tmp, out)
    _CACHE[key] = ctypes.CDLL(out)
    return _CACHE[key]
