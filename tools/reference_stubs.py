"""
Stand-ins that let the fixture tools (make_add_noise_fixture.py, make_stats_fixture.py, make_script_fixtures.py) import the
reference's script modules where the packages those modules never use on the driven path are not installed.

  * ``Stub``: a module any name can be imported from; the names are classes that take any arguments, return themselves from any
    call or attribute, and combine with ``|`` (``Usage(__doc__) | TrainData.usage`` in a class body);
  * ``Wavio``: wavio's ``read`` / ``write`` over a dict of int16 arrays instead of files -- ``load_audio`` gets the int16 array
    it was asked for, ``save_audio`` leaves the int16 array it made;
  * ``install_stubs(names)``: a ``Stub`` for every name that does not import (dotted names after their parents), -> the names
    stubbed, for the fixture's ``provenance``.

Nothing here computes anything a fixture stores.
"""
import sys
import types

import numpy as np


class Stub(types.ModuleType):
    """a module any name can be imported from"""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {'__init__': lambda self, *a, **k: None, '__call__': lambda self, *a, **k: self,
                               '__getattr__': lambda self, n: self, '__or__': lambda self, other: self})


class Wavio(types.ModuleType):
    """wavio's read / write over a dict of int16 arrays instead of files"""

    def __init__(self, rate):
        super().__init__('wavio')
        self.files, self.rate = {}, rate
        self.reads = []                 # every name read() was asked for, in order
        self.written = []               # every (name, int16 array) write() was handed, in order

    def read(self, name):
        self.reads.append(name)
        return types.SimpleNamespace(data=self.files[name].reshape(-1, 1), rate=self.rate, sampwidth=2)

    def write(self, name, data, rate, sampwidth=None, scale=None):
        assert data.dtype == np.int16 and rate == self.rate and sampwidth == 2 and scale == 'none'
        self.files[name] = np.array(data)
        self.written.append((name, self.files[name]))


def install_stubs(names) -> list:
    stubbed = []
    for name in names:
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = Stub(name)
            parent, _, child = name.rpartition('.')
            if parent and isinstance(sys.modules.get(parent), Stub):
                sys.modules[parent].__dict__[child] = sys.modules[name]
            stubbed.append(name)
    return stubbed


def install_wavio(rate) -> Wavio:
    wavio = sys.modules['wavio'] = Wavio(rate)
    return wavio
