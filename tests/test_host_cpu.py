"""Host-side logic that needs no GPU: registry / config surface, state-dict contract,
locality order, C-ABI symbols, loud failure without a device."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch


def test_capi_exports_every_declared_symbol():
    """libpave_hip.so loads on a CPU-only host and exports what include/pave_hip.h declares."""
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    lib = native.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'pave_hip.h')).read()
    declared = set(re.findall(r'\b(pave_[a-z0-9_]+)\s*\(', header))
    assert declared == set(native.EXPORTED)
    for name in declared:
        assert hasattr(lib, name), name
    m = re.search(r'#define PAVE_ABI_VERSION (\d+)', header)
    assert lib.pave_abi_version() == int(m.group(1)) == native.ABI_VERSION


def test_binding_is_derived_from_the_header():
    """native.py types every entry point from include/pave_hip.h (no hand-kept argument lists): the parser on a
    header text written here, its refusal to guess, and the types the loaded library carries."""
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    vp, ci, ll, cf, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double
    text = ('#ifndef X_H_\n#define X_H_\n#include <stdint.h>\n'
            '#define PAVE_E_ARG (-1)   /* bad argument */\n#define PAVE_ABI_VERSION 7\n#define PAVE_NAME "x"\n'
            '/* int pave_hidden(size_t n); -- and a call in prose: pave_prose(1) */\n'
            'typedef struct pave_thing { const float* x; int n; } pave_thing;\n'
            'int pave_version(void);\n'
            'const char* pave_message(void);\n'
            'long long pave_bytes(long long M, int K);\n'
            'int pave_launch(const pave_thing* things, const int64_t* index, long long rows,\n'
            '                float eps, double thresh,   // a line comment with pave_other(\n'
            '                const int n, void* stream);\n'
            '#endif\n')
    functions, defines = native.parse_header(text)
    assert functions == {'pave_version': (ci, []), 'pave_message': (ctypes.c_char_p, []),
                         'pave_bytes': (ll, [ll, ci]), 'pave_launch': (ci, [vp, vp, ll, cf, cd, ci, vp])}
    assert list(functions) == ['pave_version', 'pave_message', 'pave_bytes', 'pave_launch']
    assert defines == {'PAVE_E_ARG': -1, 'PAVE_ABI_VERSION': 7}
    # nothing is guessed: an unknown scalar, a struct by value, an array, a function pointer, a definition
    for bad, named in (('int pave_a(const float* x, size_t n, void* stream);', 'size_t n'),
                       ('int pave_b(pave_thing thing, void* stream);', 'pave_thing thing'),
                       ('int pave_c(int hw[8], void* stream);', 'hw'),
                       ('unsigned pave_d(int n);', 'pave_d'),
                       ('int pave_e(void (*done)(int), void* stream);', 'pave_e'),
                       ('static inline int pave_f(int n) { return n; }', 'pave_f'),
                       ('int pave_g(int n)\n', 'pave_g')):
        with pytest.raises(native.NativeLibraryError, match=re.escape(named)):
            native.parse_header('int pave_ok(int n);\n' + bad + '\n')
    # the real header: every declaration typed, and the loaded library carries exactly those types
    build_native()
    lib = native.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    functions, defines = native.parse_header(open(os.path.join(root, 'include', 'pave_hip.h')).read())
    assert tuple(functions) == native.EXPORTED and len(functions) >= 55
    assert set(native.SIGNATURES) < set(native.EXPORTED)
    for name in native.EXPORTED:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == functions[name][1], name
        assert fn.restype is functions[name][0], name
    assert lib.pave_last_error.restype is ctypes.c_char_p and lib.pave_gemm_splitk_workspace_bytes.restype is ll
    assert lib.pave_gemm_splitk_workspace_bytes.argtypes == [ll, ci, ci]
    assert lib.pave_oks_nms_f32.argtypes == [vp, vp, vp, cd, vp, vp, ci, ci, ci, vp]
    assert native.ABI_VERSION == defines['PAVE_ABI_VERSION'] and defines['PAVE_E_ARG'] == -1
    assert (native.AUG_MAX_AUGS, native.AUG_MAX_SLOTS, native.AUG_MAX_K) == (16, 128, 64)


def test_ctypes_struct_layout_equals_the_header(tmp_path):
    """`native.GnLevel` is passed to pave_groupnorm_levels_nhwc_f32 as an array of the header's `pave_gn_level`: a
    field that drifts apart corrupts device pointers silently.  The header is compiled (gcc, as C) into a program
    that prints sizeof / offsetof of every field; ctypes must agree."""
    import shutil
    import subprocess
    from pavenet_amd import native
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in native.GnLevel._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pave_gn_level));\n'
                   + ''.join(f'  printf(" %zu", offsetof(pave_gn_level, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(native.GnLevel)
    assert got[1:] == [getattr(native.GnLevel, f).offset for f in fields]


def test_shipped_library_has_no_diagnostic_switches():
    """The kernel-form override and the timing-only ablations live in the -DPAVE_DIAG build only:
    the shipped library exports exactly the C ABI of the header, the diag build adds pave_diag_*."""
    import subprocess
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()

    def exported(path):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True,
                             check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln}
    shipped, diag = exported(native.LIB_PATH), exported(native.DIAG_LIB_PATH)
    assert not [s for s in shipped if 'diag' in s], shipped
    assert {s for s in shipped if s.startswith('pave_')} == set(native.EXPORTED)
    assert {'pave_diag_gemm_variant', 'pave_diag_enc_tile_ablate'} <= diag
    with native.diag_build(0) as dlib:
        assert native.load() is dlib
    assert native.load() is not dlib


def test_no_buffer_store_carries_a_register_scalar_offset(tmp_path):
    """A 16-byte `buffer_store` whose scalar offset is a REGISTER gets no wait state from the compiler
    in front of a VALU write of its data registers, and on gfx950 such stores wrote the NEXT
    instruction's value into part of the wave (tools/debug_encproj.py): every buffer store
    of the GEMM translation unit must carry the literal scalar offset 0 (column tiles ride the
    immediate offset).  Checked on the ISA the shipped flags produce."""
    import shutil
    import subprocess
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip('no hipcc')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    asm = tmp_path / 'gemm.s'
    subprocess.run([hipcc, '-O3', '--offload-arch=gfx950', '-std=c++17', '--cuda-device-only', '-S',
                    '-I' + os.path.join(root, 'include'), '-I' + os.path.join(root, 'pavenet_amd', 'csrc'),
                    '-o', str(asm), os.path.join(root, 'pavenet_amd', 'csrc', 'pave_gemm_dma.hip')],
                   check=True, capture_output=True)
    stores = re.findall(r'^\s*buffer_store_dword\w*\s+(.*)$', asm.read_text(), flags=re.M)
    assert len(stores) > 100, 'the epilogue stores are buffer stores'
    for ops_ in stores:
        fields = [f.strip() for f in ops_.split(',')]
        # vdata, vaddr, srsrc, soffset [modifiers]
        assert fields[3].split()[0] == '0', ops_


def test_pybind_ext_module_surface():
    """pavenet_amd._ext (csrc/pave_mmcv_ext.cpp) builds against the installed torch headers, loads
    on a CPU-only host and exposes the two entry points of mmcv._ext with the keyword names of
    pybind.cpp:737-748; a host tensor raises before any launch (ms_deform_attn_cuda.cu:221-230)."""
    from pavenet_amd.build_native import build_native, build_ext
    build_native()
    build_ext()
    from pavenet_amd import _ext, native
    fwd, bwd = _ext.ms_deform_attn_forward.__doc__, _ext.ms_deform_attn_backward.__doc__
    assert re.findall(r'(\w+): torch.Tensor', fwd) == [
        'value', 'value_spatial_shapes', 'value_level_start_index', 'sampling_locations',
        'attention_weights'] and 'im2col_step' in fwd
    assert re.findall(r'(\w+): torch.Tensor', bwd) == [
        'value', 'value_spatial_shapes', 'value_level_start_index', 'sampling_locations',
        'attention_weights', 'grad_output', 'grad_value', 'grad_sampling_loc', 'grad_attn_weight']
    assert _ext.pave_abi_version() == native.ABI_VERSION
    v = torch.zeros(1, 30, 8, 32)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        _ext.ms_deform_attn_forward(value=v, value_spatial_shapes=torch.tensor([[5, 6]]),
                                    value_level_start_index=torch.tensor([0]),
                                    sampling_locations=torch.zeros(1, 2, 8, 1, 4, 2),
                                    attention_weights=torch.zeros(1, 2, 8, 1, 4), im2col_step=64)


def test_ops_fail_loudly_without_device():
    from pavenet_amd import ops
    v = torch.zeros(1, 30, 8, 32)
    shapes = torch.tensor([[5, 6]])
    lsi = torch.tensor([0])
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        ops.ms_deform_attn_forward(v, shapes, lsi, torch.zeros(1, 2, 8, 1, 4, 2),
                                   torch.zeros(1, 2, 8, 1, 4), 64)
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        ops.deform_attn_grid_fused(v, shapes, lsi, torch.zeros(2, 384), torch.zeros(1, 2, 4, 2),
                                   T=1, n_clips=1, units_per_clip=2)


def test_capi_argument_errors():
    """Entry points validate before launching: no GPU is touched for a bad call."""
    from pavenet_amd import native
    lib = native.load()
    st = lib.pave_ms_deform_attn_forward_f32(None, None, None, None, None, None, 1, 1, 1, 1, 1, 1,
                                             1, 1, None)
    assert st == -1 and b'null pointer' in lib.pave_last_error()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    st = lib.pave_ms_deform_attn_forward_f32(p, p, p, p, p, p, 3, 1, 1, 4, 1, 1, 1, 2, None)
    assert st == -3  # batch 3 not divisible by im2col_step 2 (ms_deform_attn_cuda.cu:242-245)
    st = lib.pave_deform_attn_grid_fused_f32(p, p, p, p, p, None, None, p, None, None, 4, 4, 1, 1,
                                             10, 3, 4, 384, None, 0, 3, None)
    assert st == -1 and b'L = 4' in lib.pave_last_error()
    # a frame table without the number of slabs behind `value`, and a slab count that contradicts n_clips * T
    st = lib.pave_deform_attn_grid_fused_f32(p, p, p, p, p, None, None, p, None, None, 4, 4, 1, 1,
                                             10, 4, 4, 384, p, 0, 4, None)
    assert st == -1 and b'n_slabs' in lib.pave_last_error()
    st = lib.pave_deform_attn_pose_fused_f32(p, p, p, p, p, p, None, None, 1, 4, 3, 10, 4, 15, 4320, None, 7, 4, None)
    assert st == -1 and b'n_slabs' in lib.pave_last_error()
    # reference rows per entry: one per level, or one shared by all levels -- nothing else
    st = lib.pave_deform_attn_pose_fused_f32(p, p, p, p, p, p, None, None, 1, 4, 3, 10, 4, 15, 4320, None, 0, 2, None)
    assert st == -1 and b'ref_levels' in lib.pave_last_error()
    st = lib.pave_deform_attn_grid_fused_f32(p, p, p, p, p, None, None, p, None, None, 4, 4, 1, 1,
                                             10, 4, 4, 384, None, 0, 0, None)
    assert st == -1 and b'ref_levels' in lib.pave_last_error()
    # the listed-rows fill and the softmax merge validate their sizes without touching the device
    assert lib.pave_fill_rows_f32(p, 6, 10, p, 1, None, 6, None) == -1      # C % 4
    assert lib.pave_fill_rows_f32(p, 8, 10, None, 0, None, 8, None) == 0    # nothing to fill: no launch
    assert lib.pave_merge_softmax_partials_f32(p, p, 2, 3, 250, 8, None) == -1
    # unsupported sampler variants are refused before anything is enqueued (advisor finding, round 4)
    hw = (ctypes.c_int * 8)(16, 24, 8, 12, 4, 6, 2, 3)
    for variant in (5, 6, 13, 16, -1):
        assert lib.pave_enc_deform_attn_tile_f32(p, p, None, p, 1, 510, ctypes.cast(hw, ctypes.c_void_p), 384,
                                                 variant, None, None) != 0


def test_state_dict_contract(golden_dir):
    """Same parameter names and shapes as the reference model."""
    from pavenet_amd.models import build_model, videopose_r50_cfg
    ref = json.load(open(os.path.join(golden_dir, 'state_dict_keys.json')))
    for T, name in ((3, 'videopose_r50_t3'), (5, 'videopose_r50_t5')):
        m = build_model(videopose_r50_cfg(num_frames=T))
        mine = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert mine == ref[name]


def test_state_dict_contract_petr(golden_dir):
    from pavenet_amd.models import build_model, petr_r50_cfg
    ref = json.load(open(os.path.join(golden_dir, 'state_dict_keys.json')))
    for name, kw in (('petr_r50', dict(num_keypoints=17, head='opera.PETRHead')),
                     ('vedpose_r50', dict(num_keypoints=15, head='opera.VedPoseHeadV2'))):
        m = build_model(petr_r50_cfg(**kw))
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref[name]


def test_generalised_frame_prefixes():
    from pavenet_amd.deform_attn import frame_prefixes
    assert frame_prefixes(1) == ['']
    assert frame_prefixes(3) == ['pre_', '', 'next_']
    assert frame_prefixes(5) == ['pre_pre_', 'pre_', '', 'next_', 'next_next_']
    assert frame_prefixes(7)[0] == 'pre_pre_pre_' and frame_prefixes(7)[6] == 'next_next_next_'
    with pytest.raises(AssertionError):
        frame_prefixes(4)


def test_registry_scopes():
    from pavenet_amd import models  # noqa: F401
    from pavenet_amd import registry as Rg
    from pavenet_amd.deform_attn import (MulFramesMultiScaleDeformableAttentionNumFrames3,
                                         MultiScaleDeformableAttention)
    # 'mmcv.X' asked of an opera registry walks to the mmcv root
    assert Rg.ATTENTION.get('mmcv.MultiScaleDeformableAttention') is MultiScaleDeformableAttention
    assert Rg.ATTENTION.get('mmcv.MulFramesMultiScaleDeformableAttentionNumFrames3') is \
        MulFramesMultiScaleDeformableAttentionNumFrames3
    assert Rg.ATTENTION.get('opera.MulFramesMultiScaleDeformablePoseAttentionNumFrames3') is not None
    assert Rg.ATTENTION.get('MulFramesMultiScaleDeformablePoseAttentionNumFrames5') is not None
    assert Rg.MODELS.get('mmdet.ResNet') is not None
    assert Rg.MODELS.get('opera.VideoPoseV1') is not None
    assert Rg.TRANSFORMER_LAYER_SEQUENCE.get('mmcv.DeformableDetrTransformerDecoderV1') is not None
    assert Rg.ATTENTION.get('mmcv.DoesNotExist') is None
    with pytest.raises(KeyError):
        Rg.build_attention(dict(type='mmcv.DoesNotExist'))
    with pytest.raises(ValueError, match='divisible'):
        Rg.build_attention(dict(type='mmcv.MultiScaleDeformableAttention', embed_dims=250,
                                num_heads=8))  # test_ms_deformable_attn.py:17-24


def test_config_base_inheritance(tmp_path):
    from pavenet_amd.config import Config
    (tmp_path / 'base.py').write_text("model = dict(type='A', head=dict(n=1, m=2))\nruntime = 3\n")
    (tmp_path / 'child.py').write_text(
        "_base_ = ['./base.py']\nmodel = dict(head=dict(n=5), neck=dict(_delete_=True, k=1))\n")
    cfg = Config.fromfile(str(tmp_path / 'child.py'))
    assert cfg.model.type == 'A' and cfg.model.head.n == 5 and cfg.model.head.m == 2
    assert cfg.model.neck == dict(k=1) and cfg.runtime == 3


def test_encoder_unit_order_is_a_band_permutation():
    from pavenet_amd.locality import encoder_unit_order
    levels = [(100, 168), (50, 84), (25, 42), (13, 21)]
    S = sum(h * w for h, w in levels)
    order = encoder_unit_order(levels, 3).numpy()
    assert sorted(order.tolist()) == list(range(3 * S))
    # first eighth = top band of every frame, on every level
    first = order[:3 * S // 8]
    frames = first // S
    assert set(frames.tolist()) == {0, 1, 2}
    tok = first % S
    lvl0 = tok[tok < 100 * 168]
    assert (lvl0 // 168).max() <= 13  # rows 0..12 of 100
    assert np.array_equal(encoder_unit_order(levels, 2, mode='none').numpy(), np.arange(2 * S))


def test_reference_config_files_build(golden_dir):
    """The `model` dicts of six of the reference's own config files (as its mmcv.Config resolves them:
    tests/golden/reference_model_configs.json, oracle/gen_golden.py `configs`) go through our registry."""
    from pavenet_amd.models import build_model
    configs = json.load(open(os.path.join(golden_dir, 'reference_model_configs.json')))
    keys = json.load(open(os.path.join(golden_dir, 'state_dict_keys.json')))
    assert sorted(configs) == sorted(['videopose_r50_t3', 'videopose_r50_t5', 'videopose_swinl_t3', 'petr_r50',
                                      'petr_hrnetw48', 'vedpose_r50'])
    for name, model in configs.items():
        model.pop('init_cfg', None)
        model['backbone'].pop('init_cfg', None)
        model['train_cfg'] = None
        m = build_model(model)
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == keys[name], name


def test_kpt2json_and_checkpoint_roundtrip(tmp_path):
    from pavenet_amd.formats import kpt2json, load_checkpoint, results2json
    det = [np.array([[10., 20., 50., 80., 0.9], [1., 2., 3., 5., 0.4]], dtype=np.float32)]
    kpt = [np.arange(2 * 15 * 3, dtype=np.float32).reshape(2, 15, 3)]
    res = [(det, kpt), ([np.zeros((0, 5), np.float32)], [np.zeros((0, 15, 3), np.float32)])]
    bj, kj = kpt2json(res, img_ids=[7, 8])
    assert len(bj) == 2 and len(kj) == 2
    assert bj[0] == dict(image_id=7, bbox=[10.0, 20.0, 40.0, 60.0], score=float(np.float32(0.9)),
                         category_id=1)
    assert kj[1]['keypoints'] == list(map(float, range(45, 90))) and kj[1]['image_id'] == 7
    files = results2json(res, [7, 8], str(tmp_path / 'out'))
    assert json.load(open(files['keypoints'])) == kj
    # the reference's own PosetrackVideoPoseDataset._kpt2json gives the same lists (tests/golden/kpt2json.json,
    # oracle/gen_golden.py `kpt2json`, on these inputs)
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kpt2json.json')))
    assert bj == want['bbox'] and kj == want['keypoints']
    # checkpoint helper: 'state_dict' wrapper + DDP 'module.' prefix
    m = torch.nn.Linear(3, 2)
    torch.save(dict(state_dict={'module.' + k: v + 1 for k, v in m.state_dict().items()},
                    meta=dict(epoch=3)), tmp_path / 'c.pth')
    m2 = torch.nn.Linear(3, 2)
    ck = load_checkpoint(m2, str(tmp_path / 'c.pth'), strict=True)
    assert ck['meta']['epoch'] == 3 and torch.equal(m2.weight, m.weight + 1)


def test_rescale_size_matches_reference_pipeline_shapes():
    """1080p -> 750 x 1333 (posetrack17_video_keypoint.py:75,81 with size_divisor=1) and
    640 x 480 COCO -> 800 x 1067 padded to 800 x 1088 (coco_keypoint.py:73,79)."""
    from oracle import preprocess_ref as PR
    from pavenet_amd.preprocess import rescale_size
    assert rescale_size((1920, 1080), (1333, 800)) == (1333, 750)
    assert rescale_size((640, 480), (1333, 800)) == (1067, 800)
    for wh in ((1920, 1080), (640, 480), (333, 500), (1333, 800)):
        assert rescale_size(wh, (1333, 800)) == PR.rescale_size(wh, (1333, 800))


def test_tuned_gemm_selection_file_is_well_formed():
    """pavenet_amd/data/tunableop_gfx950.csv: the five validators PyTorch checks before it accepts
    the file, then one `op,shape,solution,ms` row per GEMM shape (no duplicates)."""
    from pavenet_amd import tuning
    rows = [r.strip().split(',') for r in open(tuning.DEFAULT_FILE) if r.strip()]
    val = {r[1]: r[2] for r in rows if r[0] == 'Validator'}
    assert set(val) == {'PT_VERSION', 'HIP_VERSION', 'HIPBLASLT_VERSION', 'GCN_ARCH_NAME',
                        'ROCBLAS_VERSION'}
    assert val['GCN_ARCH_NAME'].startswith('gfx950')
    ent = [r for r in rows if r[0] != 'Validator']
    assert len(ent) > 30 and all(len(r) == 4 and float(r[3]) > 0 for r in ent)
    assert len({(r[0], r[1]) for r in ent}) == len(ent)
    # the bench workload's FFN shapes are covered
    assert any(r[1].startswith('tn_256_625044_1024') for r in ent)


def test_gemm_mode_switch_validates():
    from pavenet_amd import bricks
    default = bricks.get_gemm_mode()
    assert default == 'bf16x3'      # the hand-written split kernels are the library default
    with pytest.raises(AssertionError):
        bricks.set_gemm_mode('tf32')
    for mode in ('bf16x3', 'bf16x2', 'bf16', 'fp16', 'native'):
        bricks.set_gemm_mode(mode)
        assert bricks.get_gemm_mode() == mode
    # host tensors never take the device GEMM path
    x, w = torch.randn(9000, 256), torch.randn(128, 256)
    bricks.set_gemm_mode('bf16x3')
    try:
        assert not bricks.split_gemm_ok(x, w)
        y = bricks.linear_rows(x, w, None, relu=True)
        assert torch.equal(y, torch.relu(x @ w.t()))
    finally:
        bricks.set_gemm_mode(default)


@pytest.mark.parametrize('mode', ['band', 'quad', 'patch', 'none'])
def test_encoder_unit_order_is_a_permutation(mode):
    """Every processing order of the encoder tokens (locality.py) visits each (frame, token) once."""
    from pavenet_amd.locality import encoder_unit_order
    levels, F = [(13, 21), (7, 11), (4, 6), (2, 3)], 3
    S = sum(h * w for h, w in levels)
    order = encoder_unit_order(levels, F, mode)
    assert order.dtype == torch.int32 and order.shape == (F * S,)
    assert torch.equal(order.long().sort()[0], torch.arange(F * S))
    if mode == 'patch':   # the first 32 level-0 units of a band form 8 x 4 pixel patches
        first = order[:32].long() % S
        ys, xs = first // 21, first % 21
        assert int(xs.max() - xs.min()) <= 7 and int(ys.max() - ys.min()) <= 3


def test_streaming_window_rule_is_the_reference_datasets():
    """f2: VideoPoseStream.window_indices == the reference dataset's auxiliary-frame rule
    (opera/datasets/posetrack_video_pose.py:578-609, PoseTrack17 branch, 1-based frame numbers):
    prev = cur - 1 except at the first frame, next = cur + 1 except at the last one."""
    from pavenet_amd.streaming import VideoPoseStream

    def reference_rule(cur, nframes):          # restated from _get_auxiliary_frames
        prev_delta, next_delta = 1, 1
        if cur == 1:
            prev_delta, next_delta = 0, 1
        if cur == nframes:
            prev_delta, next_delta = 1, 0
        return [cur - prev_delta, cur, cur + next_delta]

    for n in range(2, 9):
        wins = VideoPoseStream.window_indices(n, 3)
        assert wins == [[i - 1 for i in reference_rule(c + 1, n)] for c in range(n)]
    # T = 5 generalisation: edge replication on both sides
    assert VideoPoseStream.window_indices(4, 5) == [[0, 0, 0, 1, 2], [0, 0, 1, 2, 3], [0, 1, 2, 3, 3],
                                                    [1, 2, 3, 3, 3]]


def test_pipeline_shapes_vs_the_references_own_rescale_size(golden_dir):
    """f4, the part that CAN be pinned without cv2: resize target size, recorded scale_factor and
    padded shape against values produced by the reference's own mmcv.rescale_size /
    impad_to_multiple arithmetic (tests/golden/pipeline_shapes.json, oracle/gen_golden.py
    `pipeline`), for the product's host planner and for the oracle's."""
    import json
    from oracle import preprocess_ref as PR
    from pavenet_amd.preprocess import plan_clip
    cases = json.load(open(os.path.join(golden_dir, 'pipeline_shapes.json')))
    assert len(cases) == 60
    for c in cases:
        (w, h), scale, div = c['src_wh'], tuple(c['scale']), c['divisor']
        Hn, Wn, Hp, Wp, sf = plan_clip(h, w, scale, div)
        assert [Wn, Hn] == c['new_wh'] and [Hp, Wp] == c['pad_hw'], c
        assert list(sf) == c['scale_factor']
        assert list(PR.rescale_size((w, h), scale)) == c['new_wh']


# What integration/ms_deform_attn_pave.cpp takes from mmcv's csrc/common/pytorch_cpp_helper.hpp and
# pytorch_device_registry.hpp, restated as checks: torch's Tensor in scope, and REGISTER_DEVICE_IMPL(key, device, fn)
# accepting fn only when it has exactly the type of the entry point `key` (mmcv's registry stores fn as a pointer of
# that type) for a device `at::k<device>`.
MMCV_HELPER_STANDIN = '''#pragma once
#include <ATen/ATen.h>
using at::Tensor;
'''
MMCV_REGISTRY_STANDIN = '''#pragma once
#include <type_traits>
#include <ATen/ATen.h>
#define REGISTER_DEVICE_IMPL(key, device, fn)                                                 \\
  static_assert(std::is_same<decltype(&key), decltype(&fn)>::value,                            \\
                #fn " does not have the signature of " #key);                                 \\
  [[maybe_unused]] static const at::DeviceType key##_##device##_registered = at::k##device;
'''


def test_integration_binding_compiles(tmp_path):
    """INTEGRATION.md section 1 is a real file: integration/ms_deform_attn_pave.cpp (the
    REGISTER_DEVICE_IMPL translation unit a maintainer adds to the vendored mmcv) type-checks
    against the installed torch headers, include/pave_hip.h and a stand-in of mmcv's two helper
    headers that checks the registrations' signatures (MMCV_REGISTRY_STANDIN: the entry points are
    declared as third_party/mmcv/mmcv/ops/csrc/pytorch/ms_deform_attn.cpp:15-46 declares them)."""
    import subprocess
    from torch.utils.cpp_extension import include_paths
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    (tmp_path / 'pytorch_cpp_helper.hpp').write_text(MMCV_HELPER_STANDIN)
    (tmp_path / 'pytorch_device_registry.hpp').write_text(MMCV_REGISTRY_STANDIN)
    cmd = ['g++', '-std=c++17', '-fsyntax-only', '-D__HIP_PLATFORM_AMD__=1', '-DUSE_ROCM=1',
           '-I/opt/rocm/include', '-I' + os.path.join(root, 'include'), '-I' + str(tmp_path)] + \
          ['-I' + p for p in include_paths()] + \
          [os.path.join(root, 'integration', 'ms_deform_attn_pave.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # the stand-in refuses a registration whose signature differs from the entry point's
    bad = tmp_path / 'bad.cpp'
    bad.write_text('#include "pytorch_cpp_helper.hpp"\n#include "pytorch_device_registry.hpp"\n'
                   'Tensor entry(const Tensor& a, const int n);\nTensor impl(const Tensor& a, const long n) { return a; }\n'
                   'REGISTER_DEVICE_IMPL(entry, CUDA, impl);\n')
    r = subprocess.run(cmd[:-1] + [str(bad)], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and 'does not have the signature of entry' in r.stderr, r.stderr[-3000:]
    # the snippet quoted in INTEGRATION.md is this file's text
    doc = open(os.path.join(root, 'INTEGRATION.md')).read()
    assert 'integration/ms_deform_attn_pave.cpp' in doc


def test_launch_census_classifies_aten_operators():
    """pavenet_amd.census.LaunchCensus (what `forward_device(strict=True)`, bench.py's `fallback_ops_per_step` and the
    GPU suite's zero-fallback tests count): library compute operators (GEMM, convolution, normalisation, attention,
    pooling, top-k) are FALLBACKS, other kernels-launching operators are counted beside them, views and allocations
    are not counted at all, slow-path notes reach the running census only -- checked here on host tensors
    (device_types=('cpu',)), the classification does not depend on the device."""
    import torch
    import torch.nn.functional as F
    from pavenet_amd.census import FallbackError, LaunchCensus, note_slow_path
    lin, x = torch.nn.Linear(8, 8), torch.randn(2, 4, 8)
    note_slow_path('outside any census: dropped')
    with torch.no_grad(), LaunchCensus(device_types=('cpu',)) as c:
        y = lin(x).relu() + 1
        y.view(8, 8).transpose(0, 1).unsqueeze(0)[:, :2].expand(3, -1, -1)      # views: nothing launched
        torch.empty(4, 4).new_empty(2)                                         # allocations
        torch.stack([y, y])
        F.layer_norm(y, (8,))
        F.conv2d(torch.randn(1, 3, 8, 8), torch.randn(4, 3, 3, 3))
        F.scaled_dot_product_attention(x, x, x)
        y.topk(2)
        note_slow_path('generic kernel')
    assert c.fallback_ops['native_layer_norm'] == 1 and c.fallback_ops['convolution'] == 1
    assert c.fallback_ops['topk'] == 1
    assert any(k in c.fallback_ops for k in ('addmm', 'mm', 'bmm', 'linear'))
    assert set(c.aten_launches) >= {'relu', 'add', 'stack'}
    assert not any(k in c.aten_launches or k in c.fallback_ops for k in ('view', 'transpose', 'expand', 'empty'))
    assert dict(c.slow_paths) == {'generic kernel': 1}
    with pytest.raises(FallbackError):
        c.raise_on_fallback('test')
    with torch.no_grad(), LaunchCensus(device_types=('cuda',)) as none:      # host tensors are not the census's
        lin(x)
    assert not none.fallback_ops and not none.aten_launches
    none.raise_on_fallback('test')


def test_round_split_rule_and_token_count():
    """Host rules of round 6: ops.round_split_rows (rows of the full rounds of the chip's 512 block slots when the
    last round would be nearly empty and its rows fit the small-row forms) and bench.tokens_per_frame (S of the
    4-level pyramid of a canvas: the byte count of the encoder roofline)."""
    import importlib.util
    from pavenet_amd import ops
    assert ops.round_split_rows(3 * 22323, 1) == 65536 and ops.round_split_rows(3 * 22323, 4) == 65536
    assert ops.round_split_rows(3 * 22323, 2) == 65536                      # value-projection pairs: N = 512
    assert ops.round_split_rows(28 * 22323, 1) is None                      # last round half full
    assert ops.round_split_rows(15 * 22323, 1) is None                      # 57 tiles = 7 296 rows: beyond the small-row forms
    assert ops.round_split_rows(3 * 20906, 1) is None                       # 490 tiles: one round
    assert ops.round_split_rows(65536, 1) is None and ops.round_split_rows(65537, 1) == 65536
    old = ops.ROUND_SPLIT
    try:
        ops.ROUND_SPLIT = False
        assert ops.round_split_rows(3 * 22323, 1) is None
    finally:
        ops.ROUND_SPLIT = old
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('bench_for_test', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.tokens_per_frame(800, 1344) == 22323 == bench.S_TOKENS
    assert bench.tokens_per_frame(750, 1333) == 94 * 167 + 47 * 84 + 24 * 42 + 12 * 21 == 20906
    assert bench.algorithmic_bytes_encoder_launch(1) == 4 * 22323 * 896
