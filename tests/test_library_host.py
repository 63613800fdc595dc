"""`hip.Library`, the one binding of every shared library of csrc/: what it says when the library or the header is
missing, the environment override, and `call` / `query` / `last_error` against the host-side refusals of
libbrever_sdr.so (nothing is launched). No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from brever_amd import hip, sdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHAT = 'The test library has no fallback.'


@pytest.fixture(scope='module')
def bound():
    return hip.Library('brever_sdr.h', 'libbrever_sdr.so', 'BRV_NO_SUCH_SWITCH', WHAT)


def test_paths_and_signatures_come_from_the_arguments(bound):
    assert os.path.samefile(bound.header_path, os.path.join(ROOT, 'include', 'brever_sdr.h'))
    assert bound.path == os.path.join(ROOT, 'brever_amd', 'csrc', 'libbrever_sdr.so') == sdr.LIB_PATH
    assert bound.signatures == sdr.SIGNATURES and bound.signatures is not sdr.SIGNATURES
    assert (sdr.HEADER_PATH, sdr.lib.__name__, sdr.call.__name__) == (bound.header_path, 'lib', 'call')
    lib = bound.lib()
    assert lib is bound.lib() and lib.brv_sdr_version() >= 100
    for name, (restype, argtypes) in bound.signatures.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the modules' names are the functions of their Library object, and each library has its own
    assert hip.lib() is not lib and hip.lib() is hip.lib()
    assert hip.SIGNATURES is not sdr.SIGNATURES and 'brv_last_error' in hip.SIGNATURES


def test_a_missing_library_names_the_path_the_build_and_the_consequence():
    missing = hip.Library('brever_sdr.h', 'libbrever_no_such.so', 'BRV_NO_SUCH_SWITCH', WHAT)
    path = os.path.join(ROOT, 'brever_amd', 'csrc', 'libbrever_no_such.so')
    assert missing.path == path                                  # constructing it loads nothing
    for use in (missing.lib, missing.last_error, lambda: missing.call('brv_sdr_forward'),
                lambda: missing.query('brv_sdr_chunk')):
        with pytest.raises(RuntimeError) as info:
            use()
        assert str(info.value) == (
            f'{path} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` or '
            f'`make -C brever_amd/csrc` (needs hipcc, targets gfx950). {WHAT}')


def test_a_missing_header_is_named():
    path = os.path.join(ROOT, 'include', 'brever_no_such.h')
    with pytest.raises(RuntimeError, match='^' + re.escape(f'{path} is missing: the binding is derived from the C '
                                                           'header') + '$'):
        hip.Library('brever_no_such.h', 'libbrever_sdr.so', 'BRV_NO_SUCH_SWITCH', WHAT)


def test_the_last_error_entry_point_is_found_in_the_header_or_given(bound):
    assert bound.lib().brv_sdr_workspace_bytes(1, 8, 513) == -1
    said = bound.last_error()
    assert 'requires' in said and said == bound.lib().brv_sdr_last_error().decode() == sdr.last_error()
    args = ('brever_sdr.h', 'libbrever_sdr.so', 'BRV_NO_SUCH_SWITCH', WHAT)
    assert hip.Library(*args, last_error='brv_sdr_last_error').last_error() == said
    with pytest.raises(AttributeError):
        hip.Library(*args, last_error='brv_last_error').last_error()


def test_the_environment_selects_the_library(tmp_path):
    """The path is read when the module is imported: a child process."""
    other = tmp_path/'libbrever_sdr_other.so'
    os.symlink(sdr.LIB_PATH, other)
    code = ('import sys; sys.path.insert(0, sys.argv[1])\n'
            'from brever_amd import hip, sdr, stoi\n'
            'print(sdr.LIB_PATH); print(stoi.LIB_PATH); print(hip.LIB_PATH)\n'
            'print(sdr.lib()._name, sdr.lib().brv_sdr_version())\n'
            'try:\n    stoi.lib()\nexcept RuntimeError as e:\n    print(e)\n')
    gone = str(tmp_path/'libbrever_gone.so')
    env = dict(os.environ, BRV_SDR_LIB_PATH=str(other), BRV_STOI_LOSS_LIB_PATH=gone, BRV_LIB_PATH='')
    out = subprocess.run([sys.executable, '-c', code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[:3] == [str(other), gone, hip.LIB_PATH]          # (an empty value is no override)
    assert lines[3].split()[0] == str(other) and int(lines[3].split()[1]) >= 100
    assert lines[4].startswith(f'{gone} is missing: build it with ') and \
        lines[4].endswith('The STOI / ESTOI criteria have no CPU fallback.')


def test_call_raises_with_the_librarys_own_message(bound):
    buf = ctypes.create_string_buffer(64)            # never read: the call is refused on the host
    args = [buf, buf, buf, 1, 8, 4, 0.0, buf, buf, buf, buf, buf, buf, None]
    for call in (bound.call, sdr.call):
        with pytest.raises(RuntimeError) as info:
            call('brv_sdr_forward', None, *args[1:])
        said = bound.last_error()
        assert 'null' in said and 'x' in said
        assert str(info.value) == f'brv_sdr_forward failed with status -1: {said}'
    with pytest.raises(AttributeError):
        bound.call('brv_sdr_no_such_entry_point')
    with pytest.raises(TypeError):
        bound.call('brv_sdr_forward', *args[:-1])                # an argument short: refused by ctypes
    with pytest.raises(RuntimeError, match=r'^sizes failed with status 3: '):
        bound.check(3, 'sizes')
    assert bound.check(0, 'sizes') is None


def test_query_returns_the_value_and_raises_on_a_negative_answer(bound):
    assert bound.query('brv_sdr_workspace_bytes', 3, 17, 512) == bound.lib().brv_sdr_workspace_bytes(3, 17, 512) > 0
    assert bound.query('brv_sdr_chunk') == bound.lib().brv_sdr_chunk()
    with pytest.raises(RuntimeError) as info:
        bound.query('brv_sdr_workspace_bytes', 1, 8, 513)
    said = bound.last_error()
    assert 'requires' in said and str(info.value) == f'brv_sdr_workspace_bytes failed with status -1: {said}'
