#!/usr/bin/env python
"""optim.GroupedOptimizer's kernels without a GPU: csrc/group_optim.hip compiled by g++ against the CPU model of common.h and driven
by the optimizer class itself on CPU tensors (a subclass replaces its four ties to the GPU: device check, library, stream, pinned
upload).  Runs the device-independent checks of tests/test_group_optim_gpu.py with their bounds - the six-step scenario against
torch in float64, bit-equal repeats, layout independence, state_dict round trips with torch - for Adam and Nesterov SGD.  It
checks arithmetic, indexing and the host logic, not timing, capture or memory.

    python3 tools/simt_model/run_group_optim.py     needs g++ with C++20 (std::barrier); two minutes or so, a thread per lane"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

from ood_object_detection_amd import _lib, optim  # noqa: E402

PRELUDE = ('#include "common.h"\n'
           'typedef float f32x4 __attribute__((vector_size(16)));\n'
           'struct int4 { int x, y, z, w; };\n'
           '#undef EFFDET_EINVAL\n#define EFFDET_EINVAL (-22)\n')


def build(tmp):
    shutil.copy(os.path.join(HERE, 'common.h'), tmp)
    src = open(os.path.join(ROOT, 'ood_object_detection_amd', 'csrc', 'group_optim.hip')).read()
    with open(os.path.join(tmp, 'group_optim.cpp'), 'w') as f:
        f.write(PRELUDE + src)
    out = os.path.join(tmp, 'libgroup_model.so')
    subprocess.run(['g++', '-std=c++20', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off', '-Wno-attributes', '-o', out,
                    os.path.join(tmp, 'group_optim.cpp')], check=True)
    lib = ctypes.CDLL(out)
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.startswith('effdet_group_'):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


class ModelOptimizer(optim.GroupedOptimizer):
    lib_model = None

    def _check_params(self, params, dev):
        assert all(p.dtype == torch.float32 and p.device.type == 'cpu' for p in params)

    def _load_lib(self):
        return self.lib_model

    def _staging(self, words):
        return torch.zeros(words, dtype=torch.int32)

    def _stream(self):
        return None, False

    def _upload(self):
        self._host[:] = self._uploaded
        self._dyn.copy_(self._pinned)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ModelOptimizer.lib_model = build(tmp)
        optim.GroupedOptimizer = ModelOptimizer
        import test_group_optim_gpu as T
        T.DEV = 'cpu'
        for name in ('adam', 'sgd'):
            T.test_six_step_scenario_matches_torch(name)
            T.test_two_runs_give_the_same_bits(name)
            T.test_layout_does_not_matter(name)
            T.test_state_dict_round_trips_with_torch(name)
            print('%s: scenario, repeat, layout independence and state_dict round trips pass on the CPU model' % name)


if __name__ == '__main__':
    main()
