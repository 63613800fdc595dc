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


def test_structs_and_constants_come_from_the_header(bound):
    from brever_amd import ffnn_stream
    with open(bound.header_path) as f:
        text = f.read()
    assert bound.constants == hip.parse_constants(text) == sdr._LIB.constants and bound.structs == {}
    with open(hip.HEADER_PATH) as f:
        text = f.read()
    constants = hip.parse_constants(text)
    assert hip._LIB.constants == constants and len(constants) == 14
    assert {name: getattr(hip, name[4:]) for name in constants if name.startswith('BRV_OPT_')} == \
        {name: value for name, value in constants.items() if name.startswith('BRV_OPT_')}
    assert hip.OPT_KNOWN == 0x17ff and hip.DCCRN_STREAM_MAX_LEVELS == constants['BRV_DCCRN_STREAM_MAX_LEVELS'] == 8
    assert sorted(flag for _, flag, _ in hip._ENV_FLAGS) == sorted(
        value for name, value in constants.items() if name.startswith('BRV_OPT_') and name != 'BRV_OPT_KNOWN')
    assert hip._LIB.structs == {'brv_launch_opts': hip.LaunchOpts, 'brv_ctn_config': hip.CtnConfig,
                                'brv_dccrn_stream_config': hip.DccrnStreamConfig}
    assert ffnn_stream._LIB.structs == {'brv_ffs_config': ffnn_stream.FfsConfig}
    assert [name for name, _ in hip.CtnConfig._fields_] == [
        'filters', 'filter_length', 'bottleneck_channels', 'hidden_channels', 'skip_channels', 'kernel_size',
        'layers', 'repeats', 'output_sources', 'causal']
    cfg = hip.CtnConfig(512, 32, 128, 512, 128, 3, 8, 3, 2, 1)       # positional, as models/convtasnet.py builds it
    assert (cfg.filters, cfg.skip_channels, cfg.causal) == (512, 128, 1)
    assert hip.LaunchOpts._fields_ == [('size', ctypes.c_uint32), ('flags', ctypes.c_uint32),
                                       ('cu_eighths', ctypes.c_int32), ('wg_target', ctypes.c_int32),
                                       ('prof', ctypes.c_void_p)]


def test_struct_layouts_equal_the_compilers(tmp_path):
    """Every struct of every header: `sizeof`, and `offsetof` and size of each field, as a C++ compiler sees the
    header, against the classes derived from its text."""
    import glob
    import shutil
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    compilers = [c for c in (clang if os.path.exists(clang) else None, shutil.which('clang++'), shutil.which('g++'))
                 if c]
    assert compilers, 'no C++ compiler'
    headers = sorted(glob.glob(os.path.join(ROOT, 'include', '*.h')))
    assert len(headers) == 9
    sizes = {}
    for header in headers:
        with open(header) as f:
            text = f.read()
        structs = hip.parse_structs(text, hip.parse_constants(text))
        if not structs:
            continue
        lines = ['#include <cstddef>', '#include <cstdio>', f'#include "{header}"', 'int main() {']
        expected = []
        for name, cls in structs.items():
            sizes[name] = ctypes.sizeof(cls)
            lines.append(f'  std::printf("{name} %zu\\n", sizeof({name}));')
            expected.append(f'{name} {ctypes.sizeof(cls)}')
            for field, _ in cls._fields_:
                lines.append(f'  std::printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), '
                             f'sizeof((({name}*)0)->{field}));')
                expected.append(f'{name}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}')
        src, exe = str(tmp_path/'layout.cpp'), str(tmp_path/'layout')
        with open(src, 'w') as f:
            f.write('\n'.join(lines + ['  return 0;', '}', '']))
        for cxx in compilers:
            r = subprocess.run([cxx, '-std=c++17', src, '-o', exe], capture_output=True, text=True)
            if r.returncode == 0:
                break
        else:
            pytest.fail(f'the layout program of {header} does not compile:\n' + r.stderr)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and out.stdout.splitlines() == expected, header
    assert sizes == {'brv_launch_opts': 24, 'brv_ctn_config': 40, 'brv_dccrn_stream_config': 1592,
                     'brv_ffs_config': 336}


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
