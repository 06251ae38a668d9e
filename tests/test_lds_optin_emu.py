"""The dynamic-LDS opt-in (kernels.hpp: lds_optin) on the host-emulated build: the emulator refuses a launch with more than 64 KiB of
dynamic LDS unless hipFuncSetAttribute raised that function's limit on the CURRENT device (HIPEMU_DEVICE), as the GPU does.  Every
family therefore has to opt in once per device, not once per process.  Opt-in state lives for the whole process, so each test uses
a device number of its own (device 0 is what every other test runs on)."""
import ctypes as C

import numpy as np
import pytest
import torch

from lemo_amd import _hip, synthetic
from lemo_amd._hip import ptr
from lemo_amd.priors import (cg8p_alloc, to_cg8p, pack_conv3x3, pack_conv3x3_gmajor, pack_conv3x3_split_f16,
                             pack_conv3x3_bwd_split_f16, pack_conv3x3_wino_f16)

LIMIT = 64 * 1024                           # dynamic LDS a launch may use without an opt-in
# dynamic LDS of each launch below (the constants in lemo_amd/csrc): every one is over the limit, or the emulator would not check it
LDS_BYTES = {
    'pair': 119904,                         # conv_pair_kernels.hip CP_SMEM
    'split': 104704,                        # conv_split_kernels.hip Cv3Cfg<64, 64, 2>::SMEM_BYTES (Cin 32 would be 52,480 B: no check)
    'wino': 131104,                         # conv_wino_kernels.hip WN_SMEM
    'tail3': 114240,                        # conv_head_kernels.hip T3_SMEM
    'lds': 126976,                          # conv_kernels.hip Cv2Cfg<512, 2>::SMEM_BYTES (Cout 64)
    'lbs': 131072,                          # lbs_kernels.hip lbs_smem_bytes(nj) >= LBS_SMEM_BYTES = 128 KiB for every nj
}


def _family_calls(lib):
    """name -> zero-argument call that launches one kernel of that family into fresh output buffers: (rc, outputs)"""
    g = torch.Generator().manual_seed(11)
    H, W = 12, 16
    x = torch.randn(64, H, W, generator=g)
    w = torch.randn(64, 64, 3, 3, generator=g) * 0.06
    b = torch.randn(64, generator=g) * 0.3
    xin = to_cg8p(x)
    pf, fi = pack_conv3x3_split_f16(w.numpy())
    pf = torch.from_numpy(pf.view(np.int16))
    wt, wt2 = torch.from_numpy(pack_conv3x3(w.numpy())), torch.from_numpy(pack_conv3x3_gmajor(w.numpy()))
    uf, ui = pack_conv3x3_wino_f16(w.numpy())
    uf = torch.from_numpy(uf.view(np.int16))
    # enc_tail3: layers 2 (64 -> 32) and 1 (32 -> 32) backwards, layer 0's adjoint
    w2, w1 = torch.randn(64, 32, 3, 3, generator=g) * 0.06, torch.randn(32, 32, 3, 3, generator=g) * 0.08
    w0 = (torch.randn(32, 9, generator=g) * 0.3).contiguous()
    p2, i2 = pack_conv3x3_bwd_split_f16(w2.numpy())
    p1, i1 = pack_conv3x3_bwd_split_f16(w1.numpy())
    p2, p1 = torch.from_numpy(p2.view(np.int16)), torch.from_numpy(p1.view(np.int16))
    d3, a2, a1 = to_cg8p(torch.randn(64, H, W, generator=g) * 1e-5), to_cg8p(torch.randn(32, H, W, generator=g)), to_cg8p(torch.randn(32, H, W, generator=g))
    # all-vertex LBS forward of a synthetic model after its pose stage
    from lemo_amd.body_model import BodyModelData, DeviceBody, alloc_pose_ws
    data = BodyModelData(synthetic.make_synthetic_smplx(seed=3, V=200, F=300))
    db = DeviceBody(data, 'cpu', blend_f16=False)
    B = 5
    ws, tt, Bp = alloc_pose_ws(B, data.nj, 'cpu', False)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.3).contiguous()
    go, body, lh, rh, betas, z3, expr = r(B, 3), r(B, 63), r(B, 12), r(B, 12), r(B, 10), torch.zeros(B, 3), torch.zeros(B, 10)
    pin = _hip.PoseIn(ptr(go), ptr(body), ptr(z3), ptr(z3), ptr(z3), ptr(lh), ptr(rh), 12, ptr(betas), 10, ptr(expr))
    lib.check(lib.smplx_pose_fwd(C.byref(db.body), C.byref(pin), C.byref(ws), B, None))

    def pair():
        mid, out = cg8p_alloc(64, H, W, 'cpu'), cg8p_alloc(64, H, W, 'cpu')
        return lib.conv3x3_pair_f16(ptr(xin), ptr(pf), fi, ptr(b), None, ptr(mid), ptr(pf), fi, ptr(b), None, ptr(out), H, W, 0, None, None), (mid, out)

    def split():
        out = cg8p_alloc(64, H, W, 'cpu')
        return lib.conv3x3_mfma_split_f16(ptr(xin), ptr(pf), fi, ptr(wt), ptr(b), None, ptr(out), H, W, 64, 64, 0, None), (out,)

    def wino():
        out = cg8p_alloc(64, H, W, 'cpu')
        return lib.conv3x3_wino_f16(ptr(xin), ptr(uf), ui, ptr(wt), ptr(b), None, ptr(out), H, W, 0, None, None), (out,)

    def tail3():
        dx0 = torch.zeros(H * W)
        return lib.enc_tail3(ptr(d3), ptr(p2), i2, ptr(a2), ptr(p1), i1, ptr(a1), ptr(w0), ptr(dx0), H, W, None), (dx0,)

    def lds():
        out = cg8p_alloc(64, H, W, 'cpu')
        return lib.conv3x3_mfma_lds(ptr(xin), ptr(wt), ptr(wt2), ptr(b), None, ptr(out), H, W, 64, 64, 0, None), (out,)

    def lbs():
        v, vp = torch.zeros(B, data.V, 3), torch.zeros(B, data.V, 3)
        return lib.lbs_verts_fwd(C.byref(db.skin), ptr(tt['Xg']), Bp, ptr(tt['A']), data.nj, None, None, data.V, B, ptr(v), ptr(vp), None), (v, vp)

    return {'pair': pair, 'split': split, 'wino': wino, 'tail3': tail3, 'lds': lds, 'lbs': lbs}


def _fitter(lib, prob, markers):
    from lemo_amd.fitting import AmassTemporalFitter
    fit = AmassTemporalFitter(prob['model'], prob['vposer_w'], prob['enc_w'], prob['ids'], prob['Xmean'], prob['Xstd'], prob['B'], 'cpu',
                              full_vertices=True, lib=lib)
    fit.load_sequence(prob['seq']['init_params'], markers, prob['seq']['contact_lbl'])
    return fit


@pytest.mark.timeout(900)
def test_every_family_opts_in_on_a_second_device(emu_lib, monkeypatch):
    """each family's launcher, first on device 0, then on device 5 of the same process: returns 0 there as well and computes the
    same bits (a process-wide "done" flag would skip the opt-in on device 5, and the emulator would refuse the launch)"""
    calls = _family_calls(emu_lib)
    assert sorted(calls) == sorted(LDS_BYTES) and all(n > LIMIT for n in LDS_BYTES.values())
    monkeypatch.setenv('HIPEMU_DEVICE', '0')
    ref = {}
    for name, call in calls.items():
        rc, ref[name] = call()
        assert rc == 0, (name, rc)
        assert any(float(t.abs().max()) > 0 for t in ref[name]), name
    monkeypatch.setenv('HIPEMU_DEVICE', '5')
    wrong = {}                                           # every family is tried: name -> return code of the ones that fail
    for name, call in calls.items():
        rc, got = call()
        if rc != 0 or not all(torch.equal(a, b) for a, b in zip(got, ref[name])):
            wrong[name] = rc
    assert not wrong, ' '.join(f'{k}: rc {v}' for k, v in sorted(wrong.items()))


@pytest.mark.timeout(900)
def test_too_little_lds_fails_at_create_not_at_launch(emu_lib, monkeypatch):
    """a device with only 64 KiB of LDS per workgroup: the fit engine (variant 9: pairs, split layer, enc_tail3, all-vertex LBS) is
    refused at construction; a direct pair launch reports an error and writes nothing; the AE engine, which asks for exactly 64 KiB,
    is still created"""
    import __graft_entry__ as ge
    prob = ge.small_problem()
    _, markers = ge.oracle_for(prob)
    monkeypatch.setenv('HIPEMU_DEVICE', '6')
    monkeypatch.setenv('HIPEMU_MAX_LDS', str(LIMIT))
    with pytest.raises(_hip.LemoHipError, match='lemo_fit_create'):
        _fitter(emu_lib, prob, markers)
    rc, (mid, out) = _family_calls(emu_lib)['pair']()
    assert rc != 0 and float(mid.abs().max()) == 0.0 and float(out.abs().max()) == 0.0
    n = int(emu_lib.ae_ws_floats(18, 22))
    ws = torch.zeros(n)
    h = emu_lib.ae_create(C.byref(_hip.AeDesc(18, 22, 3e-6, ptr(ws), n)))
    assert h
    emu_lib.ae_destroy(h)


@pytest.mark.timeout(900)
def test_fit_engine_on_a_second_device_matches_device_0(emu_lib, monkeypatch):
    """a fit engine created on device 7 after one on device 0 (its create opts every family in there): one eager step, same bits"""
    import __graft_entry__ as ge
    prob = ge.small_problem()
    _, markers = ge.oracle_for(prob)
    res = []
    for dev in ('0', '7'):
        monkeypatch.setenv('HIPEMU_DEVICE', dev)
        fit = _fitter(emu_lib, prob, markers)
        fit.step(1, use_graph=False)
        res.append((fit.params75().clone(), fit.vertices().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().max()) > 0
