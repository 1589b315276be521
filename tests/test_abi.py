"""The C-ABI library builds, loads and exports every symbol include/specmi.h declares.
No compute is run here (no GPU in the build container)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from spec_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _declared_symbols():
    src = open(os.path.join(ROOT, 'include', 'specmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(specmi_[a-z0-9_]+)\s*\(', src)))


def test_header_symbols_all_exported(lib):
    from spec_amd import _lib
    declared = _declared_symbols()
    assert len(declared) >= 18
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in specmi.h but not exported'
        assert name in _lib.PROTOTYPES, f'{name} has no ctypes prototype'
    assert sorted(_lib.PROTOTYPES) == declared


def test_version_and_no_gpu_error_path(lib):
    import torch
    assert b'gfx950' in lib.specmi_version()
    if torch.cuda.is_available():
        pytest.skip('GPU present: error path for a missing device not reachable')
    h = C.c_void_p()
    rc = lib.specmi_create(C.byref(h), 0, 1)
    assert rc != 0 and not h.value
    assert b'HIP' in lib.specmi_last_error(None) or b'device' in lib.specmi_last_error(None)


def test_struct_layouts_match_header():
    from spec_amd import _lib
    assert C.sizeof(_lib.HmrOutputs) == 8 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.ProfEntry) == 48 + 48 + 3 * 8 + 8  # int + padding


def test_product_path_has_no_cpu_fallback():
    import torch
    from spec_amd import assets
    from spec_amd.modules import CameraRegressorNetwork
    m = CameraRegressorNetwork()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 224, 224))
    # the product package never imports the oracle
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'spec_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert 'import oracle' not in src and 'from oracle' not in src, f


# ---- the option surface (round 6: frozen stable list, gated experimental list) ---------------------------------------------
def _option_table(lib):
    out, i = {}, 0
    while True:
        name, d, st = C.c_char_p(), C.c_int(), C.c_int()
        if lib.specmi_option_info(i, C.byref(name), C.byref(d), C.byref(st)) != 0:
            return out
        out[name.value.decode()] = (d.value, bool(st.value))
        i += 1


STABLE = {'backbone': 50, 'num_fc_layers': 1, 'num_fc_channels': 1024, 'use_cam': 0, 'use_cam_feats': 0, 'img_res': 224, 'hrnet_use_conv': 1,
          'estimate_var': 0, 'uncertainty_activation': 0,
          'plan': 0, 'winograd': 1, 'fuse_downsample': 1, 'head_collapse': 1, 'output_ld': 0, 'angle_ld': 0, 'experimental': 0}


def test_option_table_matches_header_and_readers(lib):
    """The library's option table is the single list: its stable part is exactly the frozen set with the documented defaults, every
    name (and nothing else) is documented in include/specmi.h under the right heading, every option but ``experimental`` (the gate
    itself) has a reader ``OPT_<name>`` in the sources, and no reader names an option by a string any more.
    Default agreement needs no test: a reader is ``opt(h, OPT_<name>)`` and states no default; the list in handle.h is the only copy."""
    table = _option_table(lib)
    assert {k: v[0] for k, v in table.items() if v[1]} == STABLE
    hdr = open(os.path.join(ROOT, 'include', 'specmi.h')).read()
    a, b = hdr.index(' * STABLE ('), hdr.index(' * EXPERIMENTAL (')
    stable_doc, exp_doc = hdr[a:b], hdr[b:hdr.index('int specmi_set_option_i32')]
    quoted = lambda text: set(re.findall(r'"([a-z][a-z_0-9]*)"', text))
    for name, (_, stable) in table.items():
        assert name in quoted(stable_doc if stable else exp_doc), f'option {name} is not documented under its heading'
    assert quoted(stable_doc) - {'focal_length'} <= {k for k, v in table.items() if v[1]}, quoted(stable_doc) - set(table)
    assert quoted(exp_doc) - {'experimental'} <= {k for k, v in table.items() if not v[1]}, quoted(exp_doc) - set(table)
    csrc = os.path.join(ROOT, 'spec_amd', 'csrc')
    src = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h', '.inc'))}
    # the list itself spells SPECMI_OPT(name, ...), never OPT_name: every OPT_<name> token in the sources is a reader
    seen = set()
    for f, text in src.items():
        for name in re.findall(r'\bOPT_([a-z_0-9]+)\b', text):
            assert name in table, f'{f}: OPT_{name} is not in the table'
            seen.add(name)
    assert seen - {'experimental'} == set(table) - {'experimental'}, set(table) ^ seen
    for f, text in src.items():
        assert not re.search(r'\bopt_[if]\s*\(', text), f'{f}: a by-name opt_i( / opt_f( read remains'
        for args in re.findall(r'\bopt\s*\(([^()]*)\)', text):
            assert not quoted(args) & set(table), f'{f}: opt( is given an option name as a string: {args}'
