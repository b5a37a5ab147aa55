"""tools/mfma_streams.py: the assembly parser on a short text written for the test (no compile)."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "mfma_streams", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "mfma_streams.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

# k_planted: six MFMAs; one dependent pair (the two on v[4:7], an s_nop between them), one exposed
# burst (two ds_read_b128, lgkmcnt(0), MFMA).  The counted wait (lgkmcnt(2)), the wait for vmcnt
# alone, the MFMA behind a VALU instruction that writes its accumulator, and the lgkmcnt(0) whose
# predecessor is no LDS read are not findings.  k_plain: no MFMA at all.
ASM = """
	.text
	.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
	.protected	k_planted
	.globl	k_planted
	.p2align	8
	.type	k_planted,@function
k_planted:                              ; @k_planted
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_lshlrev_b32_e32 v0, 4, v0
	ds_read_b128 v[20:23], v0
	ds_read_b128 v[24:27], v0 offset:64
	s_waitcnt lgkmcnt(0)
	v_mfma_f32_16x16x4_f32 v[4:7], v20, v24, v[4:7]
	s_nop 1
	v_mfma_f32_16x16x4_f32 v[4:7], v21, v25, v[4:7]
	v_mfma_f32_16x16x4_f32 v[8:11], v22, v26, v[8:11]
	ds_read_b128 v[28:31], v0 offset:128
	ds_read_b128 v[32:35], v0 offset:192
	ds_read_b128 v[36:39], v0 offset:256
	s_waitcnt lgkmcnt(2)
	v_mfma_f32_16x16x4_f32 v[12:15], v28, v24, v[12:15]
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	v_accvgpr_write_b32 a0, v12
	v_accvgpr_read_b32 v40, a0
	s_waitcnt vmcnt(0)
	v_mfma_f32_16x16x4_f32 v[4:7], v23, v27, v[4:7]
	v_mov_b32_e32 v8, 0
	s_waitcnt lgkmcnt(0)
	v_mfma_f32_16x16x4_f32 v[8:11], v32, v36, v[8:11]
	global_store_dwordx4 v0, v[4:7], s[0:1]
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel k_planted
		.amdhsa_next_free_vgpr 41
	.end_amdhsa_kernel
	.text
.Lfunc_end0:
	.size	k_planted, .Lfunc_end0-k_planted
; Kernel info:
; NumSgprs: 12
; NumVgprs: 41
; NumAgprs: 1
; TotalNumVgprs: 45
; ScratchSize: 24
	.text
	.protected	k_plain
	.globl	k_plain
	.type	k_plain,@function
k_plain:                                ; @k_plain
	v_mov_b32_e32 v1, 0
	ds_read_b32 v2, v1
	s_waitcnt lgkmcnt(0)
	v_add_f32_e32 v2, v2, v2
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel k_plain
		.amdhsa_next_free_vgpr 3
	.end_amdhsa_kernel
	.text
.Lfunc_end1:
	.size	k_plain, .Lfunc_end1-k_plain
; NumVgprs: 3
; NumAgprs: 0
; ScratchSize: 0
"""


def test_planted_burst_and_pair_are_found():
    ks = M.kernels(ASM)
    assert list(ks) == ["k_planted", "k_plain"]
    body, res = ks["k_planted"]
    assert M.stream_stats(body) == dict(insts=23, mfma=6, dep_pairs=1, bursts=1, acc_moves=2)
    assert res == dict(vgpr=41, agpr=1, scratch=24)


def test_kernel_without_mfma():
    body, res = M.kernels(ASM)["k_plain"]
    assert M.stream_stats(body) == dict(insts=5, mfma=0, dep_pairs=0, bursts=0, acc_moves=0)
    assert res == dict(vgpr=3, agpr=0, scratch=0)


def test_report_prints_one_row_per_kernel(capsys):
    M.report("planted", ASM)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "# planted" and len(out) == 4
    assert out[2].split()[:8] == ["23", "6", "1", "1", "2", "41", "1", "24"] and out[2].split()[-1] == "k_planted"
