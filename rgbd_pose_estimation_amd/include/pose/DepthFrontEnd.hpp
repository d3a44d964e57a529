// pose/DepthFrontEnd.hpp -- ADDITIVE (no reference counterpart): the step before the adapters.  The reference's callers
// hand the adapters 3 x N host matrices (TestMain.cpp:145-183 fills them from Simulator.hpp); with a depth camera those
// matrices come from a depth frame.  This class keeps that production on the GPU (Part 3 of include/rgbd_pose_hip.h):
//
//   rpe::DepthFrontEnd fe;
//   fe.setDepth(depth_mm, cam);  fe.setModelFromFrame(T_cw_prev);      // previous frame becomes the model
//   fe.setDepth(next_depth_mm, cam);
//   rpe::IcpResult r = fe.icp(T_cw_guess);                              // dense projective ICP, pose refined in place
//   rpe::DepthFrontEnd::Pairs pairs = fe.pairs(T_cw_guess);             // ... or: the adapters' matrices, born in HBM
//   NormalAOPoseAdapter<float> adapter(pairs.bv, pairs.xc, pairs.nc, pairs.xw, pairs.nw);
//   fe.attach(adapter, pairs);                                          // the solvers find the arrays resident: no upload
//   nl_shinji_kneip_ransac<float>(adapter, ...);
//
// Frame-to-model tracking against a TSDF volume (KinectFusion):
//   fe.initVolume(desc);  fe.setDepthPyramid(d0, cam, 3);  fe.integrate(T0);
//   for each frame: fe.setDepthPyramid(d, cam, 3);  fe.raycast(T, cam, range, 3);  fe.icpPyramid(T, {6, 4, 3});  fe.integrate(T);
//   rpe::Mesh m = fe.mesh();                                             // the surface: marching cubes on the GPU
// ... or without the raycast, against the volume's field itself:  fe.setDepthPyramid(d, cam, 3);  fe.icpPyramidVolume(T, {6, 4, 3});  fe.integrate(T);
// A real sensor's depth is noisy (centimetres at room distances): fe.setDepthFilter(rpe::DepthFilter()) once, before the first frame
// With a registered RGB image per frame (pixel (u, v) of colour and depth see the same ray), the volume also fuses colour:
//   fe.setDepth(d, cam);  fe.setColor(rgb);  fe.integrateColor(T);  ...  fe.modelColor();  fe.meshColors();   // RGBA8, 4 bytes each
// A sensor's colour camera is a separate one (beside the depth camera, its own size and lens): fe.registerColor(rgb, rig) in setColor's place
// ... and tracking can use it: a photometric term beside ICP holds the pose where the view is one plane (a wall, a floor, a corridor)
//   for each frame: fe.setDepthPyramid(d, cam, 3);  fe.setColor(rgb);  fe.raycast(T, cam, range, 3);  fe.modelColor();
//                   fe.preparePhoto(3);  fe.icpPyramidRgbd(T, 0.01, {6, 4, 3});  fe.integrateColor(T);
// ... and a LOST tracker recovers without a pose guess: keypoints of the frame's and the model view's colour are matched by appearance
// and the RANSAC / PROSAC solvers make the pose that ICP then refines
//   rpe::RelocResult r = fe.relocalize(6 /* shinji_kneip_prosac */, 0.05, 3.0, 0.1);
//   if (r.ok) { T = r.pose;  fe.preparePhoto(3);  fe.icpPyramidRgbd(T, 0.01, {6, 4, 3}); }
// ... also when the camera has ROLLED since (tipped, shaken, picked up): fe.setDescriptor(RPE_DESC_ORIENTED) once, before any detection
// ... against ALL the keyframes it has kept, without knowing which one the camera sees (the store lives in the context)
//   at every keyframe: fe.setModelFromFrame(T);  fe.modelColorFromFrame();  fe.detectFeatures(RPE_FEAT_MODEL);  fe.addKeyframe();
//   when lost:         rpe::KeyframeRelocResult r = fe.relocalizeKeyframes(6, 0.05, 3.0, 0.1);   // r.keyframe = the one it chose
// ... and when a LOOP closes, the keyframes' poses are made consistent: linked by their own matches, refined jointly, the store rewritten
//   after addKeyframe(): fe.linkKeyframes(id);   at a loop: rpe::GraphResult g = fe.optimizeKeyframes({0.1, 0.1, 0.05, 0.05, 0.03});
//   (g.poses[k] = keyframe k's corrected pose.  No odometry edges, no robust kernel but the gate, dense host solve.)
// ... and the MAP follows: a keyframe that carries its depth is fused again at its corrected pose, all of them in one launch
//   int32_t d[3]; fe.followShift(T, 1.5, 8, d);  if (d[0] | d[1] | d[2]) { rpe::Mesh gone = fe.mesh(1, lo, hi); fe.shiftVolume(d); }   // moving volume
//   after addKeyframe(): fe.attachFrame(id);   after optimizeKeyframes(): fe.fuseKeyframes({}, {}, true, true);  rpe::Mesh m = fe.mesh();
//   (the rebuilt volume holds the keyframes only, not the frames between them)
//
// Camera: the simulator's pinhole (Simulator.hpp:150-162).  Poses cross this interface as Sophus::SE3<double>.
#ifndef RPE_DEPTH_FRONT_END_HEADER
#define RPE_DEPTH_FRONT_END_HEADER

#include "PoseAdapterBase.hpp"

namespace rpe {

struct PinholeCamera {
  double fx = 585., fy = 585., cx = 320., cy = 240.;   // Simulator.hpp:160-162, SimpleMain.cpp:42
  int width = 640, height = 480;
};
// metres = raw value * scale; vertices outside (dmin, dmax) are invalid; normals are dropped across jumps > max_jump
struct DepthRange {
  double scale, dmin, dmax, max_jump;
  static DepthRange millimetres() { return DepthRange{0.001, 0.3, 8.0, 0.1}; }   // the usual uint16 sensor frame
  static DepthRange metres() { return DepthRange{1.0, 0.3, 8.0, 0.1}; }
};
struct IcpOptions {
  int kind = RPE_RES_P2PLANE;
  int max_iter = 10;
  double tol = 1e-6, dist_thr = 0.1, cos_thr = 0.9;
  // fused + host update = ONE resident launch for the whole loop (the fastest form: 11 us per round at 640 x 480); device_resident =
  // true
  // keeps solve and update on the GPU instead (also one launch, the grid iterates by itself: 12 us per round; no busy host thread)
  bool use_normals = true, device_resident = false, fused = true;
};
// bilateral filter on the metric depth of every later setDepth / setDepthPyramid (rpe_frame_set_filter): a (2 radius + 1)^2 window,
// Gaussian in space (sigma_space pixels), biweight in range with the cut-off depth_cut + depth_cut_z2 z^2 metres; radius 0 = off
struct DepthFilter {
  int radius = 3;
  double sigma_space = 2.0, depth_cut = 0.01, depth_cut_z2 = 0.02;
  static DepthFilter off() { DepthFilter f; f.radius = 0; return f; }
};
// a SEPARATE colour camera beside the depth camera (rpe_color_rig, for DepthFrontEnd::registerColor): its own pinhole and size, its lens
// distortion k1 k2 p1 p2 k3, the pose depth camera -> colour camera (Xk = R Xd + t), the limit on x^2 + y^2 before distortion (0 = none),
// the z-buffer cell of the occlusion test in colour pixels (0 = no test) and its tolerance occl_tol + occl_tol_z2 z^2 metres
struct ColorRig {
  PinholeCamera cam;
  double dist[5] = {0, 0, 0, 0, 0};
  SE3<double> T_kd;
  double r2_max = 0;
  int cell = 2;
  double occl_tol = 0.02, occl_tol_z2 = 0.01;
};
// TSDF volume (rpe_volume_init): dim[0] x dim[1] x dim[2] voxels of voxel_size metres from the world corner origin
struct VolumeDesc {
  int dim[3] = {256, 256, 256};
  double voxel_size = 0.02, origin[3] = {-2.56, -2.56, -0.5}, trunc = 0.06;
  int max_weight = 64;
};
// a triangle mesh of the volume's zero level set (DepthFrontEnd::mesh): 3 x V vertices and normals (world frame; NaN normals where
// the field is unknown), 3 x T vertex ids, wound so that (v1 - v0) x (v2 - v0) points to free space
struct Mesh {
  MatrixX<float> vertices, normals;
  std::vector<int32_t> triangles;
};
struct IcpResult { int iterations = 0; double last_step = 0, cost = 0; long long pairs = 0; };
// coarse-to-fine ICP: rounds run per level (0 = finest); the rest as IcpResult, of level 0
struct PyramidIcpResult : IcpResult { int level_iterations[RPE_MAX_LEVELS] = {0, 0, 0, 0}; };
// ICP with the photometric term: cost / pairs are the geometric ones, as icp reports them; the photometric ones beside them
struct RgbdIcpResult : PyramidIcpResult { double photo_cost = 0; long long photo_pairs = 0; };

// keypoint detection (rpe_features_detect) and matching (rpe_features_match) options; the defaults are the C ABI's
struct FeatureOptions { int threshold = 12, max_keypoints = RPE_MAX_KEYPOINTS; };
struct MatchOptions { int max_dist = 64, ratio_num = 8, ratio_den = 10; bool cross_check = false; };
// relocalize(): ok = false when fewer than min_matches matches were found (pose is then the identity); iterations = the solver's
// adapted Iter, votes its consensus; masks = 3 x matches shorts (2D-3D | 3D-3D | normal rows), as rpe_run returns them
struct RelocResult {
  bool ok = false;
  SE3<double> pose;
  int matches = 0, iterations = 0, votes = 0;
  std::vector<short> masks;
};
// relocalizeKeyframes(): RelocResult against the winning keyframe of the store; ok = false: keyframe / matches are the best-ranked one's
struct KeyframeRelocResult : RelocResult { int keyframe = -1; };
// queryKeyframes(): per keyframe the matches the frame would have against it, and the ids by (count descending, id ascending)
struct KeyframeRanking { std::vector<int> counts, order; };
// optimizeKeyframes(): the pose of every keyframe and, per round run, the counted pairs, the cost and |delta|; ok = false: the joint
// system was not positive definite and nothing was changed
struct GraphResult {
  bool ok = false;
  std::vector<SE3<double> > poses;
  std::vector<int64_t> pairs;
  std::vector<double> cost, step;
};
// keyframeAttachment(): what a keyframe carries for fuseKeyframes -- its level-0 metric depth (NaN = invalid), the camera it was taken
// with and, if color, its RGBA8 image; depth = false: nothing is attached
struct KeyframeAttachment {
  bool depth = false, color = false;
  PinholeCamera cam;
  std::vector<float> z;
  std::vector<uint8_t> rgba;
};

class DepthFrontEnd {
 public:
  typedef SE3<double> Pose;
  struct Pairs {            // the five adapter matrices, index = frame pixel; unpaired pixels are NaN columns of xc / bv / nc
    MatrixX<float> bv, xc, nc, xw, nw;
    long long count = 0;
  };

  explicit DepthFrontEnd(int device = Settings::get().device) : _ctx(nullptr), _device(device), _pixels(0) {
    check(rpe_create(&_ctx, device, nullptr), "rpe_create");
  }
  ~DepthFrontEnd() { if (_ctx) rpe_destroy(_ctx); }
  DepthFrontEnd(const DepthFrontEnd&) = delete;
  DepthFrontEnd& operator=(const DepthFrontEnd&) = delete;

  void setDepth(const unsigned short* depth, const PinholeCamera& cam,
      const DepthRange& r = DepthRange::millimetres()) { set(depth, RPE_DEPTH_U16, cam, r); }
  void setDepth(const float* depth, const PinholeCamera& cam,
      const DepthRange& r = DepthRange::metres()) { set(depth, RPE_DEPTH_F32, cam, r); }
  // the frame plus its coarse-to-fine pyramid of `levels` levels (rpe_frame_set_depth_pyramid)
  void setDepthPyramid(const unsigned short* depth, const PinholeCamera& cam, int levels,
      const DepthRange& r = DepthRange::millimetres()) { set(depth, RPE_DEPTH_U16, cam, r, levels); }
  void setDepthPyramid(const float* depth, const PinholeCamera& cam, int levels,
      const DepthRange& r = DepthRange::metres()) { set(depth, RPE_DEPTH_F32, cam, r, levels); }
  // denoise the depth of every LATER frame before its maps are built (a sensor's noise is centimetres at room distances: the normals
  // of raw depth are mostly noise); the current frame is not touched.  setDepthFilter(DepthFilter::off()) turns it off again
  void setDepthFilter(const DepthFilter& f) {
    const rpe_depth_filter d = {f.radius, f.sigma_space, f.depth_cut, f.depth_cut_z2};
    check(rpe_frame_set_filter(_ctx, &d), "rpe_frame_set_filter");
  }
  DepthFilter depthFilter() const {
    rpe_depth_filter d;
    check(rpe_frame_get_filter(_ctx, &d), "rpe_frame_get_filter");
    DepthFilter f;
    f.radius = d.radius; f.sigma_space = d.sigma_space; f.depth_cut = d.depth_cut; f.depth_cut_z2 = d.depth_cut_z2;
    return f;
  }
  // levels 1 .. levels-1 of the model from its level 0 (for a model given by setModel)
  void buildModelPyramid(int levels) { check(rpe_model_build_pyramid(_ctx, levels), "rpe_model_build_pyramid"); }
  // the current frame, seen from T_cw, becomes the model the next frames are registered against
  void setModelFromFrame(const Pose& T_cw) {
    double p[12]; pose12(T_cw, p);
    check(rpe_model_from_frame(_ctx, p), "rpe_model_from_frame");
  }
  void setModel(const MatrixX<float>& vertex_w, const MatrixX<float>& normal_w, const PinholeCamera& cam, const Pose& T_cw) {
    double p[12]; pose12(T_cw, p);
    const rpe_camera k = cam_of(cam);
    if (vertex_w.cols() != cam.width * cam.height || normal_w.cols() != vertex_w.cols()) throw DeviceError(RPE_ERR_ARG,
        "setModel: maps must be 3 x width*height");
    check(rpe_model_upload(_ctx, vertex_w.data(), normal_w.data(), &k, p), "rpe_model_upload");
  }
  MatrixX<float> map(int which) const {
    MatrixX<float> m(3, _pixels);
    check(rpe_frame_download(_ctx, which, m.data()), "rpe_frame_download");
    return m;
  }
  // one map of one pyramid level: RPE_MAP_* (3 x w_l*h_l) or RPE_MAP_DEPTH (1 x w_l*h_l metres)
  MatrixX<float> map(int which, int level) const {
    rpe_camera k;
    const bool model = which == RPE_MAP_MODEL_VERTEX || which == RPE_MAP_MODEL_NORMAL;
    check(rpe_frame_level_camera(_ctx, level, model ? 1 : 0, &k), "rpe_frame_level_camera");
    MatrixX<float> m(which == RPE_MAP_DEPTH ? 1 : 3, k.width * k.height);
    check(rpe_frame_download_level(_ctx, which, level, m.data()), "rpe_frame_download_level");
    return m;
  }
  long long associate(const Pose& guess, double dist_thr = 0.1, double cos_thr = 0.9, bool use_normals = true) {
    double p[12]; pose12(guess, p);
    int64_t m = 0;
    check(rpe_associate(_ctx, p, dist_thr, cos_thr, use_normals ? 1 : 0, &m), "rpe_associate");
    return (long long)m;
  }
  // dense ICP from `pose` (in/out)
  IcpResult icp(Pose& pose, const IcpOptions& o = IcpOptions()) {
    double p[12]; pose12(pose, p);
    const rpe_icp_options opt = options_of(o);
    IcpResult r;
    int64_t m = 0;
    check(rpe_icp(_ctx, &opt, p, &r.iterations, &r.last_step, &r.cost, &m), "rpe_icp");
    r.pairs = (long long)m;
    pose = pose_of(p);
    return r;
  }
  // coarse-to-fine ICP from `pose` (in/out): iters[l] rounds and gate dist_thr[l] at level l (0 = finest; dist_thr empty: o.dist_thr)
  PyramidIcpResult icpPyramid(Pose& pose, const std::vector<int>& iters, const std::vector<double>& dist_thr = std::vector<double>(),
                              const IcpOptions& o = IcpOptions()) {
    return pyramidIcp<PyramidIcpResult>("icpPyramid", "rpe_icp_pyramid", pose, iters, dist_thr, o,
        [&](const rpe_icp_options* opt, int levels, const double* gates, double* p, PyramidIcpResult& r, int64_t* m) {
          return rpe_icp_pyramid(_ctx, opt, levels, iters.data(), gates, p, r.level_iterations, &r.last_step, &r.cost, m); });
  }
  // (re)allocate and clear the TSDF volume
  void initVolume(const VolumeDesc& d) {
    rpe_volume_desc v;
    for (int a = 0; a < 3; a++) { v.dim[a] = d.dim[a]; v.origin[a] = d.origin[a]; }
    v.voxel_size = d.voxel_size; v.trunc = d.trunc; v.max_weight = d.max_weight;
    check(rpe_volume_init(_ctx, &v), "rpe_volume_init");
    _vol = d;
    _mesh_vertices = -1;
  }
  // fuse the current frame (level 0), seen from T_cw, into the volume
  void integrate(const Pose& T_cw) {
    double p[12]; pose12(T_cw, p);
    check(rpe_volume_integrate(_ctx, p), "rpe_volume_integrate");
  }
  // the model := the volume raycast from T_cw with camera cam over camera depths (r.dmin, r.dmax), plus its pyramid of `levels`
  void raycast(const Pose& T_cw, const PinholeCamera& cam, const DepthRange& r, int levels = 1) {
    double p[12]; pose12(T_cw, p);
    const rpe_camera k = cam_of(cam);
    check(rpe_volume_raycast(_ctx, p, &k, r.dmin, r.dmax), "rpe_volume_raycast");
    if (levels > 1) buildModelPyramid(levels);
  }
  // the volume on the host: 2 x voxels floats {tsdf, weight}, voxel (i, j, k) at column (k * dim1 + j) * dim0 + i
  MatrixX<float> volume() const {
    MatrixX<float> m(2, _vol.dim[0] * _vol.dim[1] * _vol.dim[2]);
    check(rpe_volume_download(_ctx, m.data()), "rpe_volume_download");
    return m;
  }
  // replace the volume's voxels: 2 x voxels floats {tsdf, weight}, the layout volume() returns
  void uploadVolume(const MatrixX<float>& m) {
    if (m.rows() != 2 || (long long)m.cols() != (long long)_vol.dim[0] * _vol.dim[1] * _vol.dim[2])
      throw DeviceError(RPE_ERR_ARG, "uploadVolume: expected 2 x voxels floats");
    check(rpe_volume_upload(_ctx, m.data()), "rpe_volume_upload");
  }
  // marching cubes over the volume, corners with weight >= min_weight (rpe_volume_mesh), brought to the host
  Mesh mesh(double min_weight = 1) const {
    int64_t nv = 0, nt = 0;
    _mesh_vertices = -1;
    check(rpe_volume_mesh(_ctx, min_weight, &nv, &nt), "rpe_volume_mesh");
    _mesh_vertices = nv;
    Mesh M;
    M.vertices.resize(3, (int)nv);
    M.normals.resize(3, (int)nv);
    M.triangles.resize((size_t)nt * 3);
    check(rpe_volume_mesh_download(_ctx, M.vertices.data(), M.normals.data(), M.triangles.data()), "rpe_volume_mesh_download");
    return M;
  }
  // the same over the cubes lo <= (i, j, k) < hi only (rpe_volume_mesh_box; 0 <= lo <= hi <= dim - 1): what a shift is about to lose
  Mesh mesh(double min_weight, const int32_t lo[3], const int32_t hi[3]) const {
    int64_t nv = 0, nt = 0;
    _mesh_vertices = -1;
    check(rpe_volume_mesh_box(_ctx, min_weight, lo, hi, &nv, &nt), "rpe_volume_mesh_box");
    _mesh_vertices = nv;
    Mesh M;
    M.vertices.resize(3, (int)nv);
    M.normals.resize(3, (int)nv);
    M.triangles.resize((size_t)nt * 3);
    check(rpe_volume_mesh_download(_ctx, M.vertices.data(), M.normals.data(), M.triangles.data()), "rpe_volume_mesh_download");
    return M;
  }
  // move the volume's window by (di, dj, dk) whole voxels along +x, +y, +z (rpe_volume_shift): new voxel (i, j, k) := old voxel
  // (i + di, j + dj, k + dk) where that was inside, cleared elsewhere, the colour volume likewise; a non-zero shift drops the last mesh
  void shiftVolume(const int32_t shift[3]) {
    check(rpe_volume_shift(_ctx, shift), "rpe_volume_shift");
    if (shift[0] || shift[1] || shift[2]) _mesh_vertices = -1;
  }
  // the volume archive (rpe_volume_archive): a pool of `capacity` bricks of 8 x 8 x 8 voxels on the device; while it is on, shiftVolume
  // takes multiples of 8, keeps every non-zero brick that leaves and restores every archived brick the window returns over.  A larger
  // capacity grows the pool, 0 switches the archive off and frees it
  void archiveVolume(int64_t capacity) { check(rpe_volume_archive(_ctx, capacity), "rpe_volume_archive"); }
  // the bricks held; capacity, if given, receives the pool's slots
  int64_t archiveHeld(int64_t* capacity = nullptr) const {
    int64_t held = 0;
    check(rpe_volume_archive_info(_ctx, &held, capacity), "rpe_volume_archive_info");
    return held;
  }
  // the held bricks sorted by (bz, by, bx): coords = 3 per brick (bx, by, bz), tsdf = 8 x 8 x 8 x 2 floats per brick in (z, y, x) order,
  // colour (may be null) = 8 x 8 x 8 x 4 binary16 per brick, zeros where none was kept; returns the number of bricks
  int64_t archiveDownload(std::vector<int64_t>& coords, std::vector<float>& tsdf, std::vector<uint16_t>* colour = nullptr) const {
    const int64_t n = archiveHeld();
    coords.assign((size_t)n * 3, 0);
    tsdf.assign((size_t)n * 1024, 0.f);
    if (colour) colour->assign((size_t)n * 2048, 0);
    check(rpe_volume_archive_download(_ctx, coords.data(), tsdf.data(), colour ? colour->data() : nullptr), "rpe_volume_archive_download");
    return n;
  }
  // forget every archived brick, keep the pool (to correct them after a loop closure instead, rebuild the map with fuseKeyframesMap)
  void archiveClear() { check(rpe_volume_archive_clear(_ctx), "rpe_volume_archive_clear"); }
  // the world-voxel bounding box of the window and every archived brick, in multiples of 8 (rpe_volume_map_bounds)
  void mapBounds(int64_t lo[3], int64_t hi[3]) const { check(rpe_volume_map_bounds(_ctx, lo, hi), "rpe_volume_map_bounds"); }
  // marching cubes over the map -- the window plus the archived bricks -- inside the box lo <= w < hi of world voxels (multiples of 8;
  // both null: the bounds), brought to the host: bit for bit the mesh of a dense volume of the box, in brick order
  // (rpe_volume_map_mesh).  meshColors() works after it
  Mesh meshMap(double min_weight = 1, const int64_t* lo = nullptr, const int64_t* hi = nullptr) const {
    int64_t nv = 0, nt = 0;
    _mesh_vertices = -1;
    check(rpe_volume_map_mesh(_ctx, min_weight, lo, hi, &nv, &nt), "rpe_volume_map_mesh");
    _mesh_vertices = nv;
    Mesh M;
    M.vertices.resize(3, (int)nv);
    M.normals.resize(3, (int)nv);
    M.triangles.resize((size_t)nt * 3);
    check(rpe_volume_mesh_download(_ctx, M.vertices.data(), M.normals.data(), M.triangles.data()), "rpe_volume_mesh_download");
    return M;
  }
  // the model := the map -- the window plus the archived bricks -- raycast from T_cw with camera cam over camera depths (r.dmin, r.dmax)
  // inside the box lo <= w < hi of world voxels (multiples of 8; both null: the bounds), plus its pyramid of `levels`: bit for bit
  // raycast() of a dense volume of the box (rpe_volume_map_raycast).  flags: RPE_MAPRAY_COLOR samples the model colour in the same pass
  // (modelColorMap() returns it); RPE_MAPRAY_NO_SKIP, the default here, leaves the occupancy pre-pass out: it changes no bit and, as
  // measured, does not pay for reading the whole window (pass 0 to run it)
  void raycastMap(const Pose& T_cw, const PinholeCamera& cam, const DepthRange& r, int levels = 1, const int64_t* lo = nullptr,
                  const int64_t* hi = nullptr, int flags = RPE_MAPRAY_NO_SKIP) {
    double p[12]; pose12(T_cw, p);
    const rpe_camera k = cam_of(cam);
    check(rpe_volume_map_raycast(_ctx, p, &k, r.dmin, r.dmax, lo, hi, flags), "rpe_volume_map_raycast");
    if (levels > 1) buildModelPyramid(levels);
  }
  // where the window is now: the descriptor of initVolume with its origin moved by the total shift (total, if given, receives it)
  VolumeDesc volumeGeometry(int64_t total[3] = nullptr) const {
    rpe_volume_desc v;
    check(rpe_volume_geometry(_ctx, &v, total), "rpe_volume_geometry");
    VolumeDesc d;
    for (int a = 0; a < 3; a++) { d.dim[a] = v.dim[a]; d.origin[a] = v.origin[a]; }
    d.voxel_size = v.voxel_size; d.trunc = v.trunc; d.max_weight = v.max_weight;
    return d;
  }
  // the shift, in multiples of `granule` voxels, that re-centres the window on the point look_ahead metres in front of the camera at
  // T_cw (rpe_volume_follow); nothing is applied: hand it to shiftVolume
  void followShift(const Pose& T_cw, double look_ahead, int granule, int32_t shift[3]) const {
    double p[12]; pose12(T_cw, p);
    check(rpe_volume_follow(_ctx, p, look_ahead, granule, shift), "rpe_volume_follow");
  }
  // the current frame's colour: width*height*3 bytes (RPE_COLOR_RGB8 or RPE_COLOR_BGR8 order) registered to its depth; a new depth
  // drops it
  void setColor(const uint8_t* rgb, int format = RPE_COLOR_RGB8) { check(rpe_frame_set_color(_ctx, rgb, format), "rpe_frame_set_color"); }
  // the current frame's colour from a SEPARATE colour camera: rgb = rig.cam.width * height * 3 bytes as that camera delivers them.  Every
  // depth pixel gets the colour its vertex projects to (A = 255), or 0 0 0 0 where it has none: outside the image, without depth, or
  // hidden from the colour camera by something nearer.  count = true: returns the number of A = 255 pixels (one host wait), else -1
  int64_t registerColor(const uint8_t* rgb, const ColorRig& rig, int format = RPE_COLOR_RGB8, bool count = false) {
    rpe_color_rig r;
    r.cam = cam_of(rig.cam);
    for (int i = 0; i < 5; i++) r.dist[i] = rig.dist[i];
    pose12(rig.T_kd, r.pose12);
    r.r2_max = rig.r2_max; r.cell = rig.cell; r.occl_tol = rig.occl_tol; r.occl_tol_z2 = rig.occl_tol_z2;
    int64_t known = -1;
    check(rpe_frame_register_color(_ctx, rgb, format, &r, count ? &known : nullptr), "rpe_frame_register_color");
    return known;
  }
  // integrate(T_cw) plus the frame's colour fused into the voxels inside the truncation band
  void integrateColor(const Pose& T_cw) {
    double p[12]; pose12(T_cw, p);
    check(rpe_volume_integrate_color(_ctx, p), "rpe_volume_integrate_color");
  }
  // the colour field at the model's level-0 vertices (after raycast / setModel / setModelFromFrame): 4 x width*height bytes RGBA8,
  // A = 255 where the colour is known, 0 0 0 0 where it is not
  std::vector<uint8_t> modelColor() const {
    rpe_camera k;
    check(rpe_model_sample_color(_ctx), "rpe_model_sample_color");
    check(rpe_frame_level_camera(_ctx, 0, 1, &k), "rpe_frame_level_camera");
    std::vector<uint8_t> out((size_t)k.width * k.height * 4);
    check(rpe_color_download(_ctx, RPE_COLOR_MODEL, out.data()), "rpe_color_download");
    return out;
  }
  // the model colour map as the device holds it, nothing sampled: what raycastMap with RPE_MAPRAY_COLOR left (modelColor() would replace
  // it with the WINDOW's colour field), or any other model colour
  std::vector<uint8_t> modelColorMap() const {
    rpe_camera k;
    check(rpe_frame_level_camera(_ctx, 0, 1, &k), "rpe_frame_level_camera");
    std::vector<uint8_t> out((size_t)k.width * k.height * 4);
    check(rpe_color_download(_ctx, RPE_COLOR_MODEL, out.data()), "rpe_color_download");
    return out;
  }
  // the colour field at the vertices of the last mesh(): 4 x n_vertices bytes RGBA8, bit for bit the model colour at the same points
  std::vector<uint8_t> meshColors() const {
    std::vector<uint8_t> out((size_t)(_mesh_vertices > 0 ? _mesh_vertices : 0) * 4);
    check(rpe_volume_mesh_colors(_ctx, out.empty() ? nullptr : out.data()), "rpe_volume_mesh_colors");
    return out;
  }
  // the model colour given by the caller (4 x width*height bytes RGBA8 at the model's level-0 size, A = 0: unknown), for a model
  // given by setModel
  void setModelColor(const uint8_t* rgba) { check(rpe_model_color_upload(_ctx, rgba), "rpe_model_color_upload"); }
  // model colour := the current frame colour, after setModelFromFrame (frame-to-frame RGB-D odometry)
  void modelColorFromFrame() { check(rpe_model_color_from_frame(_ctx), "rpe_model_color_from_frame"); }
  // the photometric maps of `levels` levels from the frame colour and the model colour; a new depth, colour, model or model colour
  // drops them
  void preparePhoto(int levels = 1) { check(rpe_photo_prepare(_ctx, levels), "rpe_photo_prepare"); }
  // icp with the photometric term beside point-to-plane (weight in metres per intensity level), one launch per round, host-driven:
  // o.kind must be RPE_RES_P2PLANE, o.device_resident false; o.fused is not consulted
  RgbdIcpResult icpRgbd(Pose& pose, double weight = 0.01, const IcpOptions& o = IcpOptions()) {
    double p[12]; pose12(pose, p);
    const rpe_icp_options opt = options_of(o);
    RgbdIcpResult r;
    int64_t m = 0, pm = 0;
    check(rpe_icp_rgbd(_ctx, &opt, weight, p, &r.iterations, &r.last_step, &r.cost, &m, &r.photo_cost, &pm), "rpe_icp_rgbd");
    r.level_iterations[0] = r.iterations;
    r.pairs = (long long)m; r.photo_pairs = (long long)pm;
    pose = pose_of(p);
    return r;
  }
  // icpPyramid with the photometric term
  RgbdIcpResult icpPyramidRgbd(Pose& pose, double weight, const std::vector<int>& iters,
                               const std::vector<double>& dist_thr = std::vector<double>(), const IcpOptions& o = IcpOptions()) {
    int64_t pm = 0;
    RgbdIcpResult r = pyramidIcp<RgbdIcpResult>("icpPyramidRgbd", "rpe_icp_pyramid_rgbd", pose, iters, dist_thr, o,
        [&](const rpe_icp_options* opt, int levels, const double* gates, double* p, RgbdIcpResult& res, int64_t* m) {
          return rpe_icp_pyramid_rgbd(_ctx, opt, weight, levels, iters.data(), gates, p, res.level_iterations, &res.last_step, &res.cost, m,
                                      &res.photo_cost, &pm); });
    r.photo_pairs = (long long)pm;
    return r;
  }
  // the residual image of a level under `pose`: model intensity at the pixel's projection minus the frame's (intensity levels), NaN
  // where the pixel has no photometric pair (row 0 of rpe_photo_rows)
  std::vector<float> photoResiduals(const Pose& pose, int level = 0, double dist_thr = 0.1) const {
    double p[12]; pose12(pose, p);
    rpe_camera k;
    check(rpe_frame_level_camera(_ctx, level, 0, &k), "rpe_frame_level_camera");
    const size_t n = (size_t)k.width * k.height;
    std::vector<float> rows(7 * n);
    check(rpe_photo_rows(_ctx, level, p, dist_thr, rows.data()), "rpe_photo_rows");
    rows.resize(n);
    return rows;
  }
  // ---- the volume term: the frame tracked against the TSDF volume ITSELF -- no raycast, no model (rpe_icp_sdf).  Of o: max_iter, tol,
  // dist_thr, cos_thr and use_normals are read; o.device_resident must be false.  The basin is the truncation band: start within a few
  // voxels of the truth (the previous frame's pose does), or let a coarse level or icp bring the pose there first
  IcpResult icpVolume(Pose& pose, const IcpOptions& o = IcpOptions()) {
    double p[12]; pose12(pose, p);
    const rpe_icp_options opt = options_of(o);
    IcpResult r;
    int64_t m = 0;
    check(rpe_icp_sdf(_ctx, &opt, p, &r.iterations, &r.last_step, &r.cost, &m), "rpe_icp_sdf");
    r.pairs = (long long)m;
    pose = pose_of(p);
    return r;
  }
  // ... coarse to fine over the frame's levels, as icpPyramid: iters[l] rounds and gate dist_thr[l] at level l
  PyramidIcpResult icpPyramidVolume(Pose& pose, const std::vector<int>& iters, const std::vector<double>& dist_thr = std::vector<double>(),
                                    const IcpOptions& o = IcpOptions()) {
    return pyramidIcp<PyramidIcpResult>("icpPyramidVolume", "rpe_icp_pyramid_sdf", pose, iters, dist_thr, o,
        [&](const rpe_icp_options* opt, int levels, const double* gates, double* p, PyramidIcpResult& r, int64_t* m) {
          return rpe_icp_pyramid_sdf(_ctx, opt, levels, iters.data(), gates, p, r.level_iterations, &r.last_step, &r.cost, m); });
  }
  // the residual image of a level under `pose`: the signed distance [m] of every frame vertex to the fused surface, NaN where the
  // pixel has no row (row 0 of rpe_sdf_rows)
  std::vector<float> volumeResiduals(const Pose& pose, int level = 0, const IcpOptions& o = IcpOptions()) const {
    double p[12]; pose12(pose, p);
    rpe_camera k;
    check(rpe_frame_level_camera(_ctx, level, 0, &k), "rpe_frame_level_camera");
    const size_t n = (size_t)k.width * k.height;
    std::vector<float> rows(7 * n);
    check(rpe_sdf_rows(_ctx, level, p, o.dist_thr, o.cos_thr, o.use_normals ? 1 : 0, rows.data()), "rpe_sdf_rows");
    rows.resize(n);
    return rows;
  }
  // ---- the volume colour term: icpVolume / icpPyramidVolume with a photometric term against the COLOUR VOLUME beside the geometric one
  // (weight in metres per intensity level): where geometry leaves the pose open -- a wall, a floor -- the colour holds it, still without
  // raycast, model or preparePhoto (rpe_icp_sdf_rgbd).  Needs setColor on the frame and a volume fused with integrateColor
  RgbdIcpResult icpVolumeColor(Pose& pose, double weight = 0.01, const IcpOptions& o = IcpOptions()) {
    double p[12]; pose12(pose, p);
    const rpe_icp_options opt = options_of(o);
    RgbdIcpResult r;
    int64_t m = 0, pm = 0;
    check(rpe_icp_sdf_rgbd(_ctx, &opt, weight, p, &r.iterations, &r.last_step, &r.cost, &m, &r.photo_cost, &pm), "rpe_icp_sdf_rgbd");
    r.level_iterations[0] = r.iterations;
    r.pairs = (long long)m; r.photo_pairs = (long long)pm;
    pose = pose_of(p);
    return r;
  }
  RgbdIcpResult icpPyramidVolumeColor(Pose& pose, double weight, const std::vector<int>& iters,
                                      const std::vector<double>& dist_thr = std::vector<double>(), const IcpOptions& o = IcpOptions()) {
    int64_t pm = 0;
    RgbdIcpResult r = pyramidIcp<RgbdIcpResult>("icpPyramidVolumeColor", "rpe_icp_pyramid_sdf_rgbd", pose, iters, dist_thr, o,
        [&](const rpe_icp_options* opt, int levels, const double* gates, double* p, RgbdIcpResult& res, int64_t* m) {
          return rpe_icp_pyramid_sdf_rgbd(_ctx, opt, weight, levels, iters.data(), gates, p, res.level_iterations, &res.last_step, &res.cost, m,
                                          &res.photo_cost, &pm); });
    r.photo_pairs = (long long)pm;
    return r;
  }
  // the residual image of a level under `pose`: the colour volume's luma at every frame vertex minus the frame's intensity (intensity
  // levels), NaN where the pixel has no photometric row (row 0 of rpe_sdf_photo_rows)
  std::vector<float> volumeColorResiduals(const Pose& pose, int level = 0, double dist_thr = 0.1) const {
    double p[12]; pose12(pose, p);
    rpe_camera k;
    check(rpe_frame_level_camera(_ctx, level, 0, &k), "rpe_frame_level_camera");
    const size_t n = (size_t)k.width * k.height;
    std::vector<float> rows(7 * n);
    check(rpe_sdf_photo_rows(_ctx, level, p, dist_thr, rows.data()), "rpe_sdf_photo_rows");
    rows.resize(n);
    return rows;
  }
  // ---- the map volume term: icpVolume / icpPyramidVolume / volumeResiduals against the whole MAP -- the window plus the archived
  // bricks -- inside the box lo <= w < hi of world voxels (multiples of 8; both null: the bounds): a surface the window has left still
  // gives rows (rpe_icp_map_sdf).  The tracked frame of a moving window with the archive on: followVolume -> shiftVolume ->
  // icpPyramidMap -> integrate
  IcpResult icpMap(Pose& pose, const IcpOptions& o = IcpOptions(), const int64_t* lo = nullptr, const int64_t* hi = nullptr) {
    double p[12]; pose12(pose, p);
    const rpe_icp_options opt = options_of(o);
    IcpResult r;
    int64_t m = 0;
    check(rpe_icp_map_sdf(_ctx, &opt, lo, hi, p, &r.iterations, &r.last_step, &r.cost, &m), "rpe_icp_map_sdf");
    r.pairs = (long long)m;
    pose = pose_of(p);
    return r;
  }
  PyramidIcpResult icpPyramidMap(Pose& pose, const std::vector<int>& iters, const std::vector<double>& dist_thr = std::vector<double>(),
                                 const IcpOptions& o = IcpOptions(), const int64_t* lo = nullptr, const int64_t* hi = nullptr) {
    return pyramidIcp<PyramidIcpResult>("icpPyramidMap", "rpe_icp_pyramid_map_sdf", pose, iters, dist_thr, o,
        [&](const rpe_icp_options* opt, int levels, const double* gates, double* p, PyramidIcpResult& r, int64_t* m) {
          return rpe_icp_pyramid_map_sdf(_ctx, opt, levels, iters.data(), gates, lo, hi, p, r.level_iterations, &r.last_step, &r.cost, m); });
  }
  std::vector<float> mapResiduals(const Pose& pose, int level = 0, const IcpOptions& o = IcpOptions(), const int64_t* lo = nullptr,
                                  const int64_t* hi = nullptr) const {
    double p[12]; pose12(pose, p);
    rpe_camera k;
    check(rpe_frame_level_camera(_ctx, level, 0, &k), "rpe_frame_level_camera");
    const size_t n = (size_t)k.width * k.height;
    std::vector<float> rows(7 * n);
    check(rpe_map_sdf_rows(_ctx, level, p, o.dist_thr, o.cos_thr, o.use_normals ? 1 : 0, lo, hi, rows.data()), "rpe_map_sdf_rows");
    rows.resize(n);
    return rows;
  }
  // ---- the map volume colour term: icpVolumeColor / icpPyramidVolumeColor / volumeColorResiduals against the whole MAP -- the TSDF and
  // the colour of the window plus the archived bricks -- inside the box (as icpMap's): a textured surface the window has left still
  // holds the in-plane motion (rpe_icp_map_sdf_rgbd).  The colour-tracked frame of a moving window with the archive on: followVolume ->
  // shiftVolume -> icpPyramidMapColor -> integrateColor
  RgbdIcpResult icpMapColor(Pose& pose, double weight = 0.01, const IcpOptions& o = IcpOptions(), const int64_t* lo = nullptr,
                            const int64_t* hi = nullptr) {
    double p[12]; pose12(pose, p);
    const rpe_icp_options opt = options_of(o);
    RgbdIcpResult r;
    int64_t m = 0, pm = 0;
    check(rpe_icp_map_sdf_rgbd(_ctx, &opt, weight, lo, hi, p, &r.iterations, &r.last_step, &r.cost, &m, &r.photo_cost, &pm), "rpe_icp_map_sdf_rgbd");
    r.level_iterations[0] = r.iterations;
    r.pairs = (long long)m; r.photo_pairs = (long long)pm;
    pose = pose_of(p);
    return r;
  }
  RgbdIcpResult icpPyramidMapColor(Pose& pose, double weight, const std::vector<int>& iters,
                                   const std::vector<double>& dist_thr = std::vector<double>(), const IcpOptions& o = IcpOptions(),
                                   const int64_t* lo = nullptr, const int64_t* hi = nullptr) {
    int64_t pm = 0;
    RgbdIcpResult r = pyramidIcp<RgbdIcpResult>("icpPyramidMapColor", "rpe_icp_pyramid_map_sdf_rgbd", pose, iters, dist_thr, o,
        [&](const rpe_icp_options* opt, int levels, const double* gates, double* p, RgbdIcpResult& res, int64_t* m) {
          return rpe_icp_pyramid_map_sdf_rgbd(_ctx, opt, weight, levels, iters.data(), gates, lo, hi, p, res.level_iterations, &res.last_step,
                                              &res.cost, m, &res.photo_cost, &pm); });
    r.photo_pairs = (long long)pm;
    return r;
  }
  std::vector<float> mapColorResiduals(const Pose& pose, int level = 0, double dist_thr = 0.1, const int64_t* lo = nullptr,
                                       const int64_t* hi = nullptr) const {
    double p[12]; pose12(pose, p);
    rpe_camera k;
    check(rpe_frame_level_camera(_ctx, level, 0, &k), "rpe_frame_level_camera");
    const size_t n = (size_t)k.width * k.height;
    std::vector<float> rows(7 * n);
    check(rpe_map_sdf_photo_rows(_ctx, level, p, dist_thr, lo, hi, rows.data()), "rpe_map_sdf_photo_rows");
    rows.resize(n);
    return rows;
  }
  // ---- the robust volume terms: a Huber or Tukey weight on the rows of icpVolume / icpMap / icpVolumeColor / icpMapColor and their
  // pyramid forms, against depth the map does not explain -- a person, a moved chair (rpe_sdf_set_robust).  Off by default; the
  // front end's own setting, it survives new frames, volumes and shifts.  kind: RPE_ROBUST_NONE / _HUBER / _TUKEY; k: the geometric
  // row's scale [m]; photo_k: the photometric row's [intensity levels, before the weight; 0: those rows at weight 1]
  struct VolumeRobust { int kind = RPE_ROBUST_NONE; double k = 0.0, photo_k = 0.0; };
  void setVolumeRobust(int kind, double k = 0.0, double photo_k = 0.0) {
    check(rpe_sdf_set_robust(_ctx, kind, k, photo_k), "rpe_sdf_set_robust");
  }
  VolumeRobust volumeRobust() const {
    VolumeRobust r;
    check(rpe_sdf_robust(_ctx, &r.kind, &r.k, &r.photo_k), "rpe_sdf_robust");
    return r;
  }
  // the weights of a level's rows under `pose` and the setting: of the geometric rows (gates of o) or, with photo, of the photometric
  // rows (gate o.dist_thr); NaN where the pixel has no row.  map: against the whole map inside the box (both null: the bounds)
  std::vector<float> volumeRobustWeights(const Pose& pose, int level = 0, const IcpOptions& o = IcpOptions(), bool photo = false,
                                         bool map = false, const int64_t* lo = nullptr, const int64_t* hi = nullptr) const {
    double p[12]; pose12(pose, p);
    rpe_camera k;
    check(rpe_frame_level_camera(_ctx, level, 0, &k), "rpe_frame_level_camera");
    std::vector<float> w((size_t)k.width * k.height);
    if (map)
      check(rpe_map_sdf_robust_weights(_ctx, level, p, o.dist_thr, o.cos_thr, o.use_normals ? 1 : 0, photo ? 1 : 0, lo, hi, w.data()),
            "rpe_map_sdf_robust_weights");
    else
      check(rpe_sdf_robust_weights(_ctx, level, p, o.dist_thr, o.cos_thr, o.use_normals ? 1 : 0, photo ? 1 : 0, w.data()),
            "rpe_sdf_robust_weights");
    return w;
  }
  // keypoints and descriptors of the frame's colour (which = RPE_FEAT_FRAME) or of the model colour (RPE_FEAT_MODEL); returns their
  // number.  A new depth, colour, model or model colour drops the side's features
  int detectFeatures(int which, const FeatureOptions& o = FeatureOptions()) {
    const rpe_feature_options fo = {o.threshold, o.max_keypoints};
    int n = 0;
    check(rpe_features_detect(_ctx, which, &fo, &n), "rpe_features_detect");
    return n;
  }
  // the descriptor of every later detection on either side, relocalize's own included: RPE_DESC_UPRIGHT (the default) or
  // RPE_DESC_ORIENTED, which survives a roll of the camera at the price of about a third of the matches without one.  A change of
  // kind drops both sides' features and the match list; a keyframe store holds one kind
  void setDescriptor(int kind) { check(rpe_features_set_descriptor(_ctx, kind), "rpe_features_set_descriptor"); }
  int descriptor() const {
    int kind = 0;
    check(rpe_features_get_descriptor(_ctx, &kind), "rpe_features_get_descriptor");
    return kind;
  }
  // the angle bins (0 .. 31, steps of 2 pi / 32) of the side's keypoints; all 0 for an upright detection
  std::vector<int32_t> featureAngles(int which) {
    std::vector<int32_t> bins((size_t)RPE_MAX_KEYPOINTS, -1);
    check(rpe_features_angles(_ctx, which, bins.data()), "rpe_features_angles");
    size_t n = 0;
    while (n < bins.size() && bins[n] >= 0) n++;
    bins.resize(n);
    return bins;
  }
  // the number of scale levels (1 .. 4: scale 1, 2/3, 1/2, 1/3) of every later detection on either side, relocalize's own included:
  // with more than one a frame taken CLOSER to the scene than its keyframe still matches it, at the price of a smaller share of correct
  // matches on a pair of one scale.  1 is the default; a change drops both sides' features and the match list.  A keyframe store may be
  // filled at one number and queried at another
  void setLevels(int levels) { check(rpe_features_set_levels(_ctx, levels), "rpe_features_set_levels"); }
  int levels() const {
    int n = 0;
    check(rpe_features_get_levels(_ctx, &n), "rpe_features_get_levels");
    return n;
  }
  // per keypoint of the side its level and its level pixel (u, v interleaved); the keypoint's own xy is the level-0 pixel it stands at
  void featureScale(int which, std::vector<int32_t>& level, std::vector<int32_t>& lxy) {
    level.assign((size_t)RPE_MAX_KEYPOINTS, -1);
    lxy.assign(2 * (size_t)RPE_MAX_KEYPOINTS, 0);
    check(rpe_features_scale(_ctx, which, level.data(), lxy.data()), "rpe_features_scale");
    size_t n = 0;
    while (n < level.size() && level[n] >= 0) n++;
    level.resize(n);
    lxy.resize(2 * n);
  }
  // match the frame's keypoints against the model's; the solver slots become the matches (n = their number, returned)
  int matchFeatures(const MatchOptions& o = MatchOptions()) {
    const rpe_match_options mo = {o.max_dist, o.ratio_num, o.ratio_den, o.cross_check ? 1 : 0};
    int m = 0;
    check(rpe_features_match(_ctx, &mo, &m), "rpe_features_match");
    return m;
  }
  // the frame's pose against the model WITHOUT a pose guess: features where missing, matches, then rpe_run's solver `method`
  // (0 .. 9) with stage `ls` on them, seeded with `seed`.  Too few matches is a result (ok = false), every other failure throws
  RelocResult relocalize(int method, double thre_3d, double thre_2d, double thre_nl, int max_iter = 200, double confidence = 0.99,
                         uint64_t seed = 1, int ls = 0, int min_matches = 12, const FeatureOptions& f = FeatureOptions(),
                         const MatchOptions& m = MatchOptions()) {
    const rpe_feature_options fo = {f.threshold, f.max_keypoints};
    const rpe_match_options mo = {m.max_dist, m.ratio_num, m.ratio_den, m.cross_check ? 1 : 0};
    RelocResult r;
    r.iterations = max_iter;
    r.masks.assign((size_t)3 * RPE_MAX_KEYPOINTS, 0);
    double p[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const int rc = rpe_relocalize(_ctx, &fo, &mo, method, thre_3d, thre_2d, thre_nl, &r.iterations, confidence, seed, ls, min_matches, p,
                                  &r.matches, &r.votes, r.masks.data());
    if (rc != RPE_ERR_DEGENERATE) check(rc, "rpe_relocalize");
    r.ok = rc == RPE_OK;
    r.masks.resize(r.ok ? (size_t)3 * r.matches : 0);
    if (r.ok) r.pose = pose_of(p);
    return r;
  }
  // the model side's current features (detectFeatures(RPE_FEAT_MODEL)) become a keyframe of the context's store; returns its id.  The
  // store survives new frames and models; clearKeyframes empties it (one keyframe cannot be removed)
  int addKeyframe() {
    int id = -1;
    check(rpe_keyframe_add(_ctx, &id), "rpe_keyframe_add");
    return id;
  }
  int keyframes() const {
    int n = 0;
    check(rpe_keyframes_count(_ctx, &n), "rpe_keyframes_count");
    return n;
  }
  void clearKeyframes() { check(rpe_keyframes_clear(_ctx), "rpe_keyframes_clear"); }
  // the frame's keypoints against every keyframe at once (needs detectFeatures(RPE_FEAT_FRAME) and a non-empty store)
  KeyframeRanking queryKeyframes(const MatchOptions& o = MatchOptions()) {
    const rpe_match_options mo = {o.max_dist, o.ratio_num, o.ratio_den, o.cross_check ? 1 : 0};
    KeyframeRanking r;
    r.counts.assign((size_t)keyframes(), 0);
    r.order.assign(r.counts.size(), 0);
    check(rpe_keyframes_query(_ctx, &mo, r.counts.data(), r.order.data()), "rpe_keyframes_query");
    return r;
  }
  // matchFeatures with keyframe `id` in the model's place
  int matchKeyframe(int id, const MatchOptions& o = MatchOptions()) {
    const rpe_match_options mo = {o.max_dist, o.ratio_num, o.ratio_den, o.cross_check ? 1 : 0};
    int m = 0;
    check(rpe_keyframe_match(_ctx, id, &mo, &m), "rpe_keyframe_match");
    return m;
  }
  // relocalize against the store: the query, then relocalize's solver run on each of the `candidates` best-ranked keyframes with at
  // least min_matches matches; the one with the most votes wins.  No keyframe with enough matches is a result (ok = false)
  KeyframeRelocResult relocalizeKeyframes(int method, double thre_3d, double thre_2d, double thre_nl, int candidates = 3, int max_iter = 200,
                                          double confidence = 0.99, uint64_t seed = 1, int ls = 0, int min_matches = 12,
                                          const FeatureOptions& f = FeatureOptions(), const MatchOptions& m = MatchOptions()) {
    const rpe_feature_options fo = {f.threshold, f.max_keypoints};
    const rpe_match_options mo = {m.max_dist, m.ratio_num, m.ratio_den, m.cross_check ? 1 : 0};
    KeyframeRelocResult r;
    r.iterations = max_iter;
    r.masks.assign((size_t)3 * RPE_MAX_KEYPOINTS, 0);
    double p[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const int rc = rpe_relocalize_keyframes(_ctx, &fo, &mo, candidates, method, thre_3d, thre_2d, thre_nl, &r.iterations, confidence, seed, ls,
                                            min_matches, p, &r.keyframe, &r.matches, &r.votes, r.masks.data());
    if (rc != RPE_ERR_DEGENERATE) check(rc, "rpe_relocalize_keyframes");
    r.ok = rc == RPE_OK;
    r.masks.resize(r.ok ? (size_t)3 * r.matches : 0);
    if (r.ok) r.pose = pose_of(p);
    return r;
  }
  // (re)build the graph's edges of the keyframes >= first against every older keyframe (first = a new keyframe's id links it alone):
  // an edge = the matches of the two keyframes' own keypoints, kept with >= min_matches pairs.  Returns the graph's edges
  int linkKeyframes(int first = 0, int min_matches = 12, const MatchOptions& o = MatchOptions()) {
    const rpe_match_options mo = {o.max_dist, o.ratio_num, o.ratio_den, o.cross_check ? 1 : 0};
    int edges = 0;
    check(rpe_keyframes_link(_ctx, first, &mo, min_matches, &edges, nullptr), "rpe_keyframes_link");
    return edges;
  }
  Pose keyframePose(int id) {
    double p[12];
    check(rpe_keyframe_info(_ctx, id, nullptr, p, nullptr, nullptr), "rpe_keyframe_info");
    return pose_of(p);
  }
  // gated Gauss-Newton over every keyframe pose, one round per gate (metres); `anchor` stays.  apply: the store takes the poses and
  // its world points move with them, so that relocalizeKeyframes answers in the corrected world
  GraphResult optimizeKeyframes(const std::vector<double>& gates, int anchor = 0, double tol = 0.0, bool apply = true) {
    GraphResult g;
    const int n = keyframes(), rounds = (int)gates.size();
    std::vector<double> p((size_t)12 * std::max(n, 1)), stats((size_t)3 * std::max(rounds, 1));
    int done = 0;
    const int rc = rpe_keyframes_optimize(_ctx, anchor, rounds, gates.data(), tol, apply ? 1 : 0, p.data(), stats.data(), &done);
    if (rc != RPE_ERR_DEGENERATE) check(rc, "rpe_keyframes_optimize");
    g.ok = rc == RPE_OK;
    if (!g.ok) return g;
    for (int k = 0; k < n; k++) g.poses.push_back(pose_of(p.data() + 12 * k));
    for (int r = 0; r < done; r++) {
      const double* st = stats.data() + (size_t)3 * r;
      g.pairs.push_back((int64_t)st[0]); g.cost.push_back(st[1]); g.step.push_back(st[2]);
    }
    return g;
  }
  // the CURRENT frame's depth, camera and (if set) colour become keyframe id's attachment: what fuseKeyframes later fuses for it.
  // Call it when the keyframe is made, while its frame is still the current one
  void attachFrame(int id) { check(rpe_keyframe_attach_frame(_ctx, id), "rpe_keyframe_attach_frame"); }
  // the same from host arrays: z = width*height metric depths (NaN = invalid), rgba = 4*width*height bytes or nullptr
  void attachKeyframe(int id, const float* z, const uint8_t* rgba, const PinholeCamera& cam) {
    const rpe_camera k = cam_of(cam);
    check(rpe_keyframe_attach_host(_ctx, id, z, rgba, &k), "rpe_keyframe_attach_host");
  }
  KeyframeAttachment keyframeAttachment(int id) {
    KeyframeAttachment a;
    int hd = 0, hc = 0;
    rpe_camera k;
    check(rpe_keyframe_attachment_info(_ctx, id, &hd, &hc, &k), "rpe_keyframe_attachment_info");
    a.depth = hd != 0; a.color = hc != 0;
    if (!a.depth) return a;
    a.cam.fx = k.fx; a.cam.fy = k.fy; a.cam.cx = k.cx; a.cam.cy = k.cy; a.cam.width = k.width; a.cam.height = k.height;
    a.z.resize((size_t)k.width * k.height);
    if (a.color) a.rgba.resize((size_t)4 * k.width * k.height);
    check(rpe_keyframe_attachment_download(_ctx, id, a.z.data(), a.color ? a.rgba.data() : nullptr), "rpe_keyframe_attachment_download");
    return a;
  }
  // the volume rebuilt from the keyframes' attachments in ONE launch, bit for bit what initVolume (clear) and one integrate /
  // integrateColor (color) per list entry leave: ids empty = every keyframe that carries depth, by id; poses empty = the store's
  // (after optimizeKeyframes: the corrected ones), else one per list entry.  The rebuilt volume holds the keyframes only, not the
  // frames between them.  cull = false switches the per-workgroup cull off (the same bits)
  void fuseKeyframes(const std::vector<int>& ids = std::vector<int>(), const std::vector<Pose>& poses = std::vector<Pose>(), bool clear = true,
                     bool color = false, bool cull = true) {
    if (!poses.empty() && poses.size() != ids.size()) throw DeviceError(RPE_ERR_ARG, "fuseKeyframes: one pose per list entry");
    std::vector<int32_t> list(ids.begin(), ids.end());
    std::vector<double> p((size_t)12 * poses.size());
    for (size_t e = 0; e < poses.size(); e++) pose12(poses[e], p.data() + 12 * e);
    const int flags = (clear ? RPE_FUSE_CLEAR : 0) | (color ? RPE_FUSE_COLOR : 0) | (cull ? 0 : RPE_FUSE_NO_CULL);
    check(rpe_volume_fuse_keyframes(_ctx, list.empty() ? nullptr : list.data(), (int)list.size(), poses.empty() ? nullptr : p.data(), flags),
          "rpe_volume_fuse_keyframes");
    if (clear) _mesh_vertices = -1;
  }
  // what fuseKeyframesMap did: bricks in the box, bricks written, archive slots newly taken, slots released
  struct MapFuseStats { int64_t bricks = 0, written = 0, archived = 0, released = 0; };
  // the whole MAP rebuilt from the keyframes: the list fused into every brick of the box lo <= w < hi of world voxels (multiples of 8;
  // both null: the map's bounds), in the window or in the archive, bit for bit what fuseKeyframes leaves in a dense volume of the box
  // that held the map's content (rpe_volume_map_fuse_keyframes).  Bricks outside the window that become non-empty take archive slots
  // (RPE_ERR_STATE, nothing written, if the pool is too small), held bricks that end empty under `clear` give theirs back.  The
  // loop-closure recipe: optimizeKeyframes -> fuseKeyframesMap(clear = true) -> meshMap
  MapFuseStats fuseKeyframesMap(const std::vector<int>& ids = std::vector<int>(), const std::vector<Pose>& poses = std::vector<Pose>(),
                                bool clear = true, bool color = false, bool cull = true, const int64_t* lo = nullptr,
                                const int64_t* hi = nullptr) {
    if (!poses.empty() && poses.size() != ids.size()) throw DeviceError(RPE_ERR_ARG, "fuseKeyframesMap: one pose per list entry");
    std::vector<int32_t> list(ids.begin(), ids.end());
    std::vector<double> p((size_t)12 * poses.size());
    for (size_t e = 0; e < poses.size(); e++) pose12(poses[e], p.data() + 12 * e);
    const int flags = (clear ? RPE_FUSE_CLEAR : 0) | (color ? RPE_FUSE_COLOR : 0) | (cull ? 0 : RPE_FUSE_NO_CULL);
    int64_t st[4] = {0, 0, 0, 0};
    check(rpe_volume_map_fuse_keyframes(_ctx, list.empty() ? nullptr : list.data(), (int)list.size(), poses.empty() ? nullptr : p.data(), flags,
                                        lo, hi, st),
          "rpe_volume_map_fuse_keyframes");
    if (clear) _mesh_vertices = -1;
    MapFuseStats out;
    out.bricks = st[0]; out.written = st[1]; out.archived = st[2]; out.released = st[3];
    return out;
  }
  // associate under `guess` and bring the five arrays to the host (the adapters' getters and the minimal solvers read them)
  Pairs pairs(const Pose& guess, double dist_thr = 0.1, double cos_thr = 0.9, bool use_normals = true) {
    Pairs P;
    P.count = associate(guess, dist_thr, cos_thr, use_normals);
    MatrixX<float>* dst[RPE_NUM_ARRAYS] = {&P.xw, &P.xc, &P.bv, &P.nw, &P.nc};
    for (int s = 0; s < RPE_NUM_ARRAYS; s++) { dst[s]->resize(3, _pixels);
        check(rpe_download(_ctx, s, dst[s]->data()), "rpe_download"); }
    return P;
  }
  // an adapter constructed over `P` runs its solvers on this front end's context: the arrays are already in HBM
  template <class Adapter> void attach(Adapter& adapter, const Pairs& P) {
    const void* host[RPE_NUM_ARRAYS] = {P.xw.data(), P.xc.data(), P.bv.data(), P.nw.data(), P.nc.data()};
    adapter.device().adopt(_ctx, _device, _pixels, RPE_F32, host);
  }
  rpe_context* context() { return _ctx; }
  int pixels() const { return _pixels; }

  static void pose12(const Pose& T, double p[12]) {
    const Matrix3<double> R = T.so3().matrix();
    for (int i = 0; i < 9; i++) p[i] = R.a[i];
    for (int i = 0; i < 3; i++) p[9 + i] = T.translation()[i];
  }
  static Pose pose_of(const double p[12]) {
    Matrix3<double> R; for (int i = 0; i < 9; i++) R.a[i] = p[i];
    const Quat<double> q = quat_from_R<double>(R.a);
    return Pose(SO3<double>::fromQuaternion(q.w, q.x, q.y, q.z), Point3<double>(p[9], p[10], p[11]));
  }

 private:
  // what the three icpPyramid* members share: one gate per level or none, the options, the pose in and out, the rounds of all levels
  // and the pairs; call(options, levels, gates or null, pose12, result, &pairs) is the entry point `entry`
  template <class Result, class Call>
  Result pyramidIcp(const char* member, const char* entry, Pose& pose, const std::vector<int>& iters, const std::vector<double>& dist_thr,
                    const IcpOptions& o, Call call) {
    if (!dist_thr.empty() && dist_thr.size() != iters.size()) throw DeviceError(RPE_ERR_ARG, std::string(member) + ": one gate per level");
    double p[12]; pose12(pose, p);
    const rpe_icp_options opt = options_of(o);
    Result r;
    int64_t m = 0;
    check(call(&opt, (int)iters.size(), dist_thr.empty() ? nullptr : dist_thr.data(), p, r, &m), entry);
    for (size_t l = 0; l < iters.size(); l++) r.iterations += r.level_iterations[l];
    r.pairs = (long long)m;
    pose = pose_of(p);
    return r;
  }
  static rpe_icp_options options_of(const IcpOptions& o) {
    rpe_icp_options opt;
    opt.kind = o.kind; opt.max_iter = o.max_iter; opt.tol = o.tol; opt.dist_thr = o.dist_thr; opt.cos_thr = o.cos_thr;
    opt.use_normals = o.use_normals; opt.device_resident = o.device_resident; opt.fused = o.fused;
    return opt;
  }
  static rpe_camera cam_of(const PinholeCamera& c) { rpe_camera k; k.fx = c.fx; k.fy = c.fy; k.cx = c.cx; k.cy = c.cy;
      k.width = c.width; k.height = c.height; return k; }
  void set(const void* depth, int type, const PinholeCamera& cam, const DepthRange& r, int levels = 1) {
    const rpe_camera k = cam_of(cam);
    if (levels == 1) check(rpe_frame_set_depth(_ctx, depth, type, &k, r.scale, r.dmin, r.dmax, r.max_jump), "rpe_frame_set_depth");
    else check(rpe_frame_set_depth_pyramid(_ctx, depth, type, &k, r.scale, r.dmin, r.dmax, r.max_jump, levels),
               "rpe_frame_set_depth_pyramid");
    _pixels = cam.width * cam.height;
  }
  rpe_context* _ctx;
  int _device, _pixels;
  VolumeDesc _vol;
  mutable int64_t _mesh_vertices = -1;   // vertices of the last mesh() (meshColors' size), -1 before one
};

}  // namespace rpe

#endif
