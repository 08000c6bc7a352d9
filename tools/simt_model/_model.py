"""What the run_*.py of the OOD and the evaluation units share: the build of one unit of csrc/ against the CPU model of common.h, and
the buffers its C ABI is driven with."""
import ctypes
import glob
import os
import shutil
import subprocess

import numpy as np

from ood_object_detection_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, 'ood_object_detection_amd', 'csrc')
PRELUDE = '''#include "common.h"
#include "effdet_hip.h"
#include <cstdint>
#undef EFFDET_EINVAL
#define EFFDET_EINVAL (-22)
using std::min; using std::floor; using std::fabs;
'''
GUARD = 64


def build(tmp, unit, prefix, lds=None):
    """csrc/<unit>.hip -> a shared library in tmp with the entry points of _lib.SIGNATURES that start with `prefix` (a string or a
    tuple of them) bound.  Every header of csrc/ is copied beside it, the model's common.h in place of the device one.  lds: (the unit's
    declaration of its dynamic LDS, the fixed-size array that stands for it)"""
    for header in glob.glob(os.path.join(CSRC, '*.h')):
        shutil.copy(header, tmp)
    shutil.copy(os.path.join(HERE, 'common.h'), tmp)
    src = open(os.path.join(CSRC, unit + '.hip')).read()
    if lds:
        assert src.count(lds[0]) == 1
        src = src.replace(*lds)
    cpp = os.path.join(tmp, unit + '.cpp')
    with open(cpp, 'w') as f:
        f.write(PRELUDE + src)
    out = os.path.join(tmp, 'lib%s_model.so' % unit)
    subprocess.run(['g++', '-std=c++20', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off', '-Wno-attributes', '-Wno-unknown-pragmas',
                    '-I', os.path.join(ROOT, 'include'), '-o', out, cpp], check=True)
    lib = ctypes.CDLL(out)
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.startswith(prefix):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


def guarded(shape, dtype, fill):
    """(view of `shape`, the whole buffer with GUARD trailing sentinels)"""
    n = int(np.prod(shape))
    whole = np.full(n + GUARD, fill, dtype)
    return whole[:n].reshape(shape), whole
