"""numpy statement of the map volume colour term of include/rgbd_pose_hip.h Part 3 ("Map volume colour term": rpe_map_sdf_photo_rows,
rpe_map_sdf_photo_normal_eq, rpe_icp_map_sdf_rgbd, rpe_icp_pyramid_map_sdf_rgbd), the contract map_sdf_photo_rows_kernel and
icp_map_sdf_photo_kernel of csrc/rpe_map_sdf_photo.hpp are held to: the rows BIT EXACTLY, the sums to sdf_photo_oracle's rounding
bound.  A composition of existing statements that restates none of them: the virtual volume AND the virtual colour volume of a box of
the map (mapmesh_oracle.dense / geometry) and the volume colour term on dense volumes (sdf_photo_oracle).  A map is (window, colour
window or None, total shift, store, kw): archive_oracle's model -- a brick held without a colour plane is held with zeros -- and the
init descriptor."""
import mapmesh_oracle as MM
import sdf_photo_oracle as SP


def virtual(window, cwindow, total, store, kw, box=None):
    """(vol, cvol, G, box): the dense virtual volume and colour volume of the box (None: the map's bounds) and their fp32 geometry"""
    d2, d1, d0 = window.shape[:3]
    box = MM.bounds(total, (d0, d1, d2), store) if box is None else box
    vol, cvol = MM.dense(window, cwindow, total, store, box)
    return vol, cvol, MM.geometry(kw, box), box


def rows(window, cwindow, total, store, kw, box, V, If, pose12, dist_thr, stages=None):
    """rpe_map_sdf_photo_rows: sdf_photo_oracle.rows on the two virtual volumes"""
    vol, cvol, G, _ = virtual(window, cwindow, total, store, kw, box)
    return SP.rows(vol, cvol, G, V, If, pose12, dist_thr, stages)


record = SP.record
combined = SP.combined


def icp_map_sdf_rgbd(oracle_lib, window, cwindow, total, store, kw, box, V, N, If, pose, iters, dist_thr, cos_thr, weight, use_normals=True,
                     tol=0.0):
    """rpe_icp_map_sdf_rgbd: sdf_photo_oracle.icp_sdf_rgbd on the virtual volumes (the map does not change inside a call)"""
    vol, cvol, G, _ = virtual(window, cwindow, total, store, kw, box)
    return SP.icp_sdf_rgbd(oracle_lib, vol, cvol, G, V, N, If, pose, iters, dist_thr, cos_thr, weight, use_normals, tol)


def icp_pyramid_map_sdf_rgbd(oracle_lib, window, cwindow, total, store, kw, box, frame_pyr, fint, pose, iters, gates, cos_thr, weight,
                             use_normals=True):
    """rpe_icp_pyramid_map_sdf_rgbd: sdf_photo_oracle.icp_pyramid_sdf_rgbd on the virtual volumes"""
    vol, cvol, G, _ = virtual(window, cwindow, total, store, kw, box)
    return SP.icp_pyramid_sdf_rgbd(oracle_lib, vol, cvol, G, frame_pyr, fint, pose, iters, gates, cos_thr, weight, use_normals)
