"""3dgp_amd -- MI355X-native generator-forward hot path of 3DGP (gfx950 HIP kernels behind a C ABI).

The directory name starts with a digit, so import it with ``importlib.import_module('3dgp_amd')``
(tests/conftest.py and the repo-root scripts do).

  config, weights      configuration + reference state-dict layout + deterministic synthetic weights (numpy only)
  _lib                 ctypes binding of csrc/libtdgp_hip.so (include/tdgp.h)
  ops                  bias_act / upfirdn2d / conv2d_resample / modulated_conv2d with the reference's signatures
  renderer             camera, rays, tri-plane field, importance sampling, ray marchers
  generator            Generator / SynthesisNetwork / MappingNetwork with the reference's state-dict names
  adaptors             DepthAdaptor / CameraAdaptor / Conv2dLayer
  metrics              FeatureStats, Frechet distance, camera priors, generator feature loop (host side)
  inference            generate / generate_trajectory / camera trajectories; shared tri-planes, uint8 video grids on the device
  compat               `src.*` module aliases so reference-style call sites resolve to this package
  distributed          batch-sharded multi-GPU generation (one process per GPU, RCCL all-gather of features)
  graphs               the whole generator forward as one captured HIP graph per (batch, options)
  geometry             density grid on the reference's voxel grid, marching cubes on the device, .obj / .ply / .mrc writers
  shapes               iso-surface depth, normals and shading straight from the rays (shape frames, uint8 video grids of them)
  mesh                 the extracted mesh rasterised from the cameras (mesh frames: visibility buffer, face or field normals, video grids)
  mesh_components      connected components of the extracted mesh: labels, per-component counts / area / volume / box, order-preserving filter
  mesh_surface         corner table of the extracted mesh: vertex normals, Taubin smoothing, open rims (smooth-shaded mesh frames, normals in .obj / .ply)
  mesh_simplify        vertex clustering of the extracted mesh with quadric placement: a tenth of the triangles, creases kept, on the device
  mesh_decimate        quadric edge collapse in rounds: N triangles or an error bound, the surface stays closed, oriented, of the same topology
  mesh_distance        how far one mesh is from another: triangle grid, closest points, sampled two-sided distance (Hausdorff, mean, RMS), error colours
  mesh_rays            what a ray hits on a mesh: first hit / any hit through the triangle grid, segment visibility, ambient occlusion per point or vertex
  mesh_texture         a per-triangle texture atlas of the extracted mesh baked from the field: textured mesh frames, .obj with vt / .mtl / .png
  mesh_build           the mesh of one sample from its planes, every stage in order: the one build behind extract_geometry and the mesh frames
  augment              the ADA augmentation pipe: per-sample parameters, geometry, colour, noise and cutout on the device, with adjoints
  step_tail            gradient pack / sanitise / norm / Adam and the EMA update as multi-tensor kernels (opt-in)
  dataset              ImageFolderDataset, InfiniteSampler, threaded batch iterator (host code: numpy + PIL)
  training_loop        the training driver: ticks, snapshots, metrics, resume (tools/train.py is its command line)
  instance_selection   the dataset filter of the ImageNet recipe: Gaussian log-likelihood scores on the fp64 matrix pipe, top-k, folder copy
  images               Pillow-exact anti-aliased resampling of uint8 images and 16-bit depth maps (device kernels + host path), detector input
  data_tools           resize_dataset / merge_depth_data / extract_features: the offline data scripts of the ImageNet recipe
"""
from . import config, weights  # noqa: F401  (numpy only)
from .config import GeneratorConfig  # noqa: F401


def __getattr__(name):
    # torch-dependent submodules are imported on first use
    if name in ('_lib', 'ops', 'renderer', 'generator', 'adaptors', 'metrics', 'inference', 'discriminator', 'training', 'compat', 'distributed', 'build', 'graphs', 'geometry', 'shapes', 'mesh', 'mesh_components', 'mesh_surface', 'mesh_simplify', 'mesh_decimate', 'mesh_distance', 'mesh_rays', 'mesh_texture', 'mesh_build', 'augment', 'step_tail', 'dataset', 'training_loop', 'instance_selection', 'images', 'data_tools'):
        import importlib
        return importlib.import_module(f'{__name__}.{name}')
    raise AttributeError(name)


def inference_golden_trajectories():
    """The trajectory configurations behind tests/golden/trajectories.npz (configs/scripts/inference.yaml style entries)."""
    return dict(point=dict(name='point', num_frames=1, yaw_offset=0.3, pitch_offset=-0.1, fov_offset=2.0),
                front_circle=dict(name='front_circle', num_frames=8, yaw_diff=0.4, pitch_diff=0.2, fov_diff=1.0),
                points=dict(name='points', yaw_offsets=[-0.5, 0.0, 0.5], pitch_offset=0.1),
                line=dict(name='line', num_frames=5, yaw_start=-0.6, yaw_end=0.6, pitch_start=1.2, pitch_end=1.8, fov=None, fov_offset=1.5))
