"""numpy statement of the map volume term of include/rgbd_pose_hip.h Part 3 ("Map volume term": rpe_map_sdf_rows,
rpe_map_sdf_normal_eq, rpe_icp_map_sdf, rpe_icp_pyramid_map_sdf), the contract map_sdf_rows_kernel and icp_map_sdf_kernel of
csrc/rpe_frontend.hip are held to: the rows BIT EXACTLY, the sums to sdf_oracle's rounding bound.  It is a composition of existing
statements and restates none of them: the virtual volume of a box of the map (mapmesh_oracle.dense / geometry) and the volume term
on a dense volume (sdf_oracle).  A map is (window, total shift, store, kw): archive_oracle's model and the init descriptor."""
import mapmesh_oracle as MM
import sdf_oracle as SO


def virtual(window, total, store, kw, box=None):
    """(vol, G, box): the dense virtual volume of the box (None: the map's bounds) and its fp32 geometry"""
    d2, d1, d0 = window.shape[:3]
    box = MM.bounds(total, (d0, d1, d2), store) if box is None else box
    return MM.dense(window, None, total, store, box)[0], MM.geometry(kw, box), box


def rows(window, total, store, kw, box, V, N, pose12, dist_thr, cos_thr, use_normals=True, stages=None):
    """rpe_map_sdf_rows: sdf_oracle.rows on the virtual volume"""
    vol, G, _ = virtual(window, total, store, kw, box)
    return SO.rows(vol, G, V, N, pose12, dist_thr, cos_thr, use_normals, stages)


record = SO.record


def icp_map_sdf(oracle_lib, window, total, store, kw, box, V, N, pose, iters, dist_thr, cos_thr, use_normals=True, tol=0.0):
    """rpe_icp_map_sdf: sdf_oracle.icp_sdf on the virtual volume (the map does not change inside a call)"""
    vol, G, _ = virtual(window, total, store, kw, box)
    return SO.icp_sdf(oracle_lib, vol, G, V, N, pose, iters, dist_thr, cos_thr, use_normals, tol)


def icp_pyramid_map_sdf(oracle_lib, window, total, store, kw, box, frame_pyr, pose, iters, gates, cos_thr, use_normals=True):
    """rpe_icp_pyramid_map_sdf: sdf_oracle.icp_pyramid_sdf on the virtual volume"""
    vol, G, _ = virtual(window, total, store, kw, box)
    return SO.icp_pyramid_sdf(oracle_lib, vol, G, frame_pyr, pose, iters, gates, cos_thr, use_normals)
