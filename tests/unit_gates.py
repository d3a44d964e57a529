"""What every compiled unit of the library must satisfy, stated once: the gate table that tests/test_isa_resources.py applies to each
entry of build.UNITS, and the three helpers the feature files share (built, exported, check_entry_points).  Data, no tests.

FLOOR holds for every kernel unit and an entry of GATES may only tighten it: no vector spills, no more than 16 bytes of scratch (the
call frame of the device-side 6x6 solve, the only out-of-line device function) and 512 registers.  PRIVATE_ARRAYS is the one wider
scratch floor: the minimal-solver generators of rpe_hypotheses.hip keep polynomial tables indexed at run time, stack arrays, not spills.
A kernel that cannot meet this is not instantiated; its launcher routes the call elsewhere (rpe_joint.hip joint_resident_fits,
rpe_normal_eq.hip normal_eq_resident_fits) and says so.  Keys of an entry:
  kernels     {base name (isa_tools.split_symbol): count}, the exact multiset of the unit's kernels; absent = no name pin
  sgpr_spill  most scalar spills of any kernel (absent = not gated)
  scratch     most bytes of private segment of any kernel
  regs        most vgpr + agpr of any kernel
  lds         {base name or "*" for every kernel: (least, most) bytes of group segment}"""
import os
import subprocess

from rgbd_pose_estimation_amd import _lib as L, build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.dirname(B.LIB)
CSRC = B.CSRC
FLOOR = dict(vgpr_spill=0, scratch=16, regs=512)
PRIVATE_ARRAYS = {"rpe_hypotheses.hip": 384}
NO_LDS = {"*": (0, 0)}
FEATURE = dict(sgpr_spill=0, scratch=0, regs=128, lds={"*": (0, 16 * 1024)})
STAGED = 14 * 13 * 13 * 8        # rpe_mapmesh.hip: the staged region of a brick, 14 x 13 x 13 voxels of 8 bytes = 18 928 B

GATES = {
    # the solver side: no name pin (hundreds of template instances), the floor alone
    "rpe_normal_eq.hip": {},
    "rpe_icp.hip": {},
    "rpe_joint.hip": {},
    "rpe_score.hip": {},
    "rpe_nl.hip": {},
    "rpe_frontend.hip": {},
    "rpe_hypotheses.hip": {},
    "rpe_prosac.hip": {},
    # one kernel, float and unsigned short raw depth.  The build shows 6 560 B of LDS ((32 + 8) rows of 41 floats) and 38 VGPRs.  Two
    # 256-thread workgroups on a CU need 2 waves per SIMD: <= 256 VGPRs each and <= 80 KiB of LDS each; 64 leaves that far behind
    "rpe_filter.hip": dict(kernels={"depth_filter_kernel": 2}, sgpr_spill=0, scratch=0, regs=64, lds={"*": (40 * 41 * 4, 40 * 41 * 4)}),
    "rpe_volume.hip": dict(kernels={"volume_integrate_kernel": 1, "volume_raycast_kernel": 1}),
    "rpe_mesh.hip": dict(kernels={"mesh_classify_kernel": 1, "mesh_count_kernel": 1, "mesh_scan_kernel": 1, "mesh_vertex_kernel": 1,
                                  "mesh_triangle_kernel": 1}),
    "rpe_color.hip": dict(kernels={"frame_color_kernel": 1, "volume_integrate_color_kernel": 1, "color_sample_kernel": 1}),
    "rpe_photo.hip": dict(kernels={"frame_intensity_kernel": 1, "model_photo_kernel": 1, "photo_rows_kernel": 1, "icp_photo_kernel": 4}),
    "rpe_feature.hip": dict(FEATURE, kernels={"feat_" + k + "_kernel": 1 for k in ("accept", "best", "compact", "describe", "gather", "nms", "scan",
                                                                                 "score", "select")}),
    # one wave per keypoint: full occupancy
    "rpe_feature_oriented.hip": dict(kernels={"feat_describe_oriented_kernel": 1}, sgpr_spill=0, scratch=0, regs=64, lds=NO_LDS),
    "rpe_feature_scale.hip": dict(FEATURE, kernels={"feat_" + k + "_kernel": 1 for k in ("compact_levels", "describe_levels",
                                                                                       "describe_oriented_levels", "nms_levels", "resample",
                                                                                       "score_levels")}),
    "rpe_keyframe.hip": dict(FEATURE, kernels={"kf_best_kernel": 1, "kf_gather_kernel": 1, "kf_rank_kernel": 1, "kf_snapshot_kernel": 1}),
    "rpe_graph.hip": dict(kernels={"graph_pack_kernel": 1, "graph_round_kernel": 1, "graph_rows_kernel": 1, "graph_apply_kernel": 1}, scratch=0),
    # the pack kernel and the four flavours of the fuse kernel (clear x colour): the registers of 4 voxels x 4 words plus one projection are few
    "rpe_rebuild.hip": dict(kernels={"volume_fuse_kernel": 4, "attach_pack_kernel": 1}, sgpr_spill=0, scratch=0, regs=128),
    "rpe_register.hip": dict(kernels={"register_splat_kernel": 1, "register_gather_kernel": 1}, scratch=0),
    # 4 pairs x 2 volumes x 4 words, their indices, little else
    "rpe_shift.hip": dict(kernels={"volume_shift_kernel": 2}, sgpr_spill=0, scratch=0, regs=64, lds=NO_LDS),
    # 4 chunks x 2 volumes x 4 words, their indices, little else
    "rpe_archive.hip": dict(kernels={"brick_occupancy_kernel": 2, "brick_copy_kernel": 5}, sgpr_spill=0, scratch=0, regs=64, lds=NO_LDS),
    # the count kernel adds its 729 case bytes to the staged region
    "rpe_mapmesh.hip": dict(kernels={"map_colour_kernel": 1, "map_count_kernel": 1, "map_scan_kernel": 1, "map_triangle_kernel": 1,
                                     "map_vertex_kernel": 1}, sgpr_spill=0, scratch=0, regs=128,
                            lds={"*": (0, 65536), "map_vertex_kernel": (STAGED, STAGED + 512), "map_count_kernel": (STAGED + 729, STAGED + 729 + 1024),
                                 "map_triangle_kernel": (0, 511), "map_colour_kernel": (0, 511)}),
}
# whole library (round 4: 401 kernels in rpe_normal_eq, 204 in rpe_joint, a 15 MB library)
MAX_KERNELS = {"rpe_normal_eq.hip": 320, "rpe_joint.hip": 160}
MAX_LIBRARY_BYTES = 10 * 1024 * 1024
# the C-ABI side is split by job (rpe_host.hpp lists the units); neither a host unit nor a header they share may grow back into a catch-all file
MAX_HOST_SOURCE_BYTES = 40 * 1024
SHARED_HOST_HEADERS = ("rpe_host.hpp", "rpe_devbuf.hpp", "rpe_gn_host.hpp", "rpe_frontend_host.hpp")


def built():
    """path of the library, built first if a source is newer"""
    return B.build()


def obj(unit):
    return os.path.join(LIB, os.path.splitext(unit)[0] + ".o")


def exported():
    """the symbols the built library exports as code"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", built()]).decode()
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def check_entry_points(syms):
    """what every feature's entry points share: exported as code, bound by _lib.py, declared `int` in the C header.  Returns the header's
    text for the feature's own assertions."""
    syms = set(syms)
    assert syms <= exported(), sorted(syms - exported())
    assert syms <= set(L.SYMBOLS), sorted(syms - set(L.SYMBOLS))
    hdr = open(os.path.join(ROOT, "include", "rgbd_pose_hip.h")).read()
    for s in sorted(syms):
        assert f"int {s}(" in hdr, s
    return hdr
