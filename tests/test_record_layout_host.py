"""Host-side half of the Python wrapper's shared rules: the packed record's one table and layout function, the joints payload
taken from that layout, the shared ``out=`` check and the producers' input validators.  No GPU, no engine."""
import inspect
import itertools
import math
import re
import types

import pytest
import torch

from spec_amd import engine, pipeline, preprocess
from spec_amd.engine import PACKED_KEYS, Engine, _image_out, record_layout


def test_layout_is_the_running_sum_of_the_table():
    lay, total = record_layout(6890)
    assert [k for k, _, _ in lay] == [k for k, _ in PACKED_KEYS]
    sizes = [math.prod(shp) for _, _, shp in lay]
    assert [off for _, off, _ in lay] == [0] + list(itertools.accumulate(sizes))[:-1]
    assert total == sum(sizes) == 21294 == 20670 + 624
    assert [shp for _, _, shp in lay[1:]] == [shp for _, shp in PACKED_KEYS[1:]] and lay[0][2] == (6890, 3)
    small, total10 = record_layout(10)
    assert total10 == 30 + 624 and small[0][2] == (10, 3)
    assert [(k, shp) for k, _, shp in small[1:]] == [(k, shp) for k, _, shp in lay[1:]]       # only the first size changes
    assert [off - 30 for _, off, _ in small[1:]] == [off - 20670 for _, off, _ in lay[1:]]


def test_the_table_is_one_object_under_all_three_names():
    import spec_amd
    assert pipeline.PACKED_KEYS is PACKED_KEYS and spec_amd.PACKED_KEYS is PACKED_KEYS
    assert pipeline.record_layout is record_layout
    got = Engine.record_layout(types.SimpleNamespace(num_verts=10))      # the method needs only num_verts
    assert isinstance(got[0], list) and got == (list(record_layout(10)[0]), 654)


def _random_outputs(B, V):
    g = torch.Generator().manual_seed(1)
    return {k: torch.randn(B, *((V, 3) if shp is None else shp), generator=g) for k, shp in PACKED_KEYS}


def test_pack_unpack_roundtrip_small_body():
    B, V = 3, 10
    out = _random_outputs(B, V)
    packed = pipeline.pack_outputs(out)
    assert packed.shape == (B, 654)
    back = pipeline.unpack_outputs(packed, V)
    assert list(back) == [k for k, _ in PACKED_KEYS]
    for k in out:
        assert back[k].shape == out[k].shape and torch.equal(back[k], out[k])


@pytest.mark.parametrize('V', [10, 6890])
def test_joints_payload_is_the_layouts_columns_after_the_vertices(V):
    B = 2
    lay, total = record_layout(V)
    start = dict((k, off) for k, off, _ in lay)['smpl_joints3d']
    assert start == 3 * V
    rec = torch.arange(B * total, dtype=torch.float32).reshape(B, total)
    views = pipeline.unpack_outputs(rec, V)
    payload = pipeline.joints_payload({'record': rec, **views})
    assert payload.is_contiguous() and torch.equal(payload, rec[:, start:total])
    assert torch.equal(payload, pipeline.joints_payload(views))                     # the same columns from separate tensors
    joints = pipeline.unpack_joints(payload)
    assert list(joints) == [k for k, _ in PACKED_KEYS[1:]]
    for k, v in joints.items():
        assert v.shape == views[k].shape and torch.equal(v, views[k])
    with pytest.raises(ValueError, match='packed record'):
        pipeline.joints_payload({'record': rec[:, 1:], **views})                    # a width no vertex count gives


@pytest.mark.parametrize('f16', [False, True])
def test_image_out_allocates_or_checks(f16):
    cpu = torch.device('cpu')
    shape, dtype = ((2, 5, 7, 8), torch.float16) if f16 else ((2, 3, 5, 7), torch.float32)
    fresh = _image_out(None, 2, 5, 7, f16, cpu)
    assert tuple(fresh.shape) == shape and fresh.dtype == dtype and fresh.is_contiguous()
    assert _image_out(fresh, 2, 5, 7, f16, cpu) is fresh
    other = torch.float32 if f16 else torch.float16
    bad = {'shape': torch.empty(2, *shape[1:-1], shape[-1] + 1, dtype=dtype), 'dtype': torch.empty(shape, dtype=other),
           'strides': torch.empty(*shape[:-1], 2 * shape[-1], dtype=dtype)[..., ::2], 'device': torch.empty(shape, dtype=dtype, device='meta')}
    assert tuple(bad['strides'].shape) == shape and not bad['strides'].is_contiguous()
    for what, t in bad.items():
        with pytest.raises(ValueError, match='out must be a contiguous'):
            _image_out(t, 2, 5, 7, f16, cpu)


def test_every_out_user_goes_through_the_shared_check():
    for fn in (preprocess._crop_outputs, preprocess.camcalib_transform_batch, Engine.resize_normalize_ragged):
        assert '_image_out(' in inspect.getsource(fn), fn.__name__
    for fn in (preprocess.crop_detections, preprocess.crop_detections_batch):
        assert '_crop_outputs(' in inspect.getsource(fn)


class _ReportsCuda(torch.Tensor):
    """A host tensor that says it lives on the GPU: lets the validators' dtype and rank checks run without one."""
    device = torch.device('cuda', 0)


@pytest.mark.parametrize('check,good,wrong_rank', [(preprocess._frame_arg, (4, 6, 3), (2, 4, 6, 3)),
                                                   (preprocess._slab_arg, (2, 4, 6, 3), (4, 6, 3))])
def test_frame_and_slab_validators(check, good, wrong_rank):
    with pytest.raises(RuntimeError, match='some_producer needs a device tensor'):
        check('some_producer', torch.zeros(good, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='some_producer needs a device tensor'):
        check('some_producer', [[0]])
    on = lambda t: t.as_subclass(_ReportsCuda)
    ok = on(torch.zeros(good, dtype=torch.uint8))
    assert check('some_producer', ok).data_ptr() == ok.data_ptr()
    for t in (torch.zeros(good, dtype=torch.float32), torch.zeros(wrong_rank, dtype=torch.uint8),
              torch.zeros(*good[:-1], 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r'some_producer: frames? must be .*uint8'):
            check('some_producer', on(t))
    if check is preprocess._slab_arg:
        with pytest.raises(ValueError, match='some_producer: frames must be a contiguous'):
            check('some_producer', on(torch.zeros(2, 4, 6, 6, dtype=torch.uint8)[..., ::2]))
    with pytest.raises(ValueError, match='dets must be'):
        preprocess._boxes_arg(torch.zeros(3, 5), 'cpu')
    assert preprocess._boxes_arg([[1, 2, 3, 4]], 'cpu').shape == (1, 4)


def test_every_producer_names_itself_to_its_validator():
    for fn, check in ((preprocess.crop_detections, '_frame_arg'), (preprocess.dataset_crops, '_frame_arg'),
                      (preprocess.camcalib_transform, '_frame_arg'), (preprocess.crop_detections_batch, '_slab_arg'),
                      (preprocess.camcalib_transform_batch, '_slab_arg')):
        assert f"{check}('{fn.__name__}'," in inspect.getsource(fn)


def test_engine_states_no_record_shape_outside_the_table():
    src = inspect.getsource(engine)
    table = re.search(r'^PACKED_KEYS = \(\n.*?^\)\n', src, flags=re.S | re.M)
    assert table is not None
    rest = src.replace(table.group(0), '')
    for literal in ('49, 3', '49, 2', '24, 3, 3', '144'):
        assert literal in table.group(0) and literal not in rest, literal


def test_feature_shape_has_one_statement():
    src = inspect.getsource(engine)
    assert src.count('o(H, 7, 2, 3)') == 1 and src.count('def o(') == 1 and '_feat_shape(' in inspect.getsource(Engine.trunk)
    assert '_feat_shape(' in inspect.getsource(Engine.trunk_pair)
    half = lambda n: -(-n // 2)
    for H, W in ((224, 224), (600, 901), (33, 1)):
        want = (H, W)
        for _ in range(5):          # the stem, the max-pool and three stride-2 stages each halve, rounding up
            want = (half(want[0]), half(want[1]))
        assert Engine._feat_shape(H, W) == want
