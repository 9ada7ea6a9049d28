"""ctypes binding of libimpact_voxel_hip.so — the exact C ABI declared in include/impact_voxel_hip.h.

This is the same surface a Rust `define_lib!` binding would see. There is no CPU
fallback anywhere in this package: if the shared library is missing or no gfx950 device is present,
calls raise `IvxError`.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IMPACT_VOXEL_HIP_LIB", os.path.join(_HERE, "lib", "libimpact_voxel_hip.so"))

IVX_OK, IVX_ERR_INVALID, IVX_ERR_HIP, IVX_ERR_CAPACITY, IVX_ERR_STATE = 0, 1, 2, 3, 4

CHUNK_INFO_DTYPE = np.dtype(
    [
        ("kind", "u1"),
        ("gen_kind", "u1"),
        ("flags", "u1"),
        ("uniform_type", "u1"),
        ("face_dist", "<u2"),
        ("region_count", "u1"),
        ("boundary_region_count", "u1"),
    ]
)
SUBMESH_DTYPE = np.dtype(
    [
        ("chunk_indices", "<u4", (3,)),
        ("index_offset", "<u4"),
        ("index_count", "<u4"),
        ("is_obscured_from_direction", "<u4", (2, 2, 2)),
        ("vertex_offset", "<u4"),
        ("vertex_count", "<u4"),
        ("reserved", "<u4"),
    ]
)
MOMENTS_DTYPE = np.dtype([("m64", "<f8", (10,)), ("m32", "<f4", (10,)), ("reserved", "<u4", (2,))])
REGION_DESC_DTYPE = np.dtype(
    [
        ("root_chunk", "<u4"),
        ("root_region", "<u4"),
        ("voxel_count", "<u8"),
        ("lo", "<u4", (3,)),
        ("hi", "<u4", (3,)),
        ("non_uniform_chunk_count", "<u4"),
        ("chunk_count", "<u4"),
        ("moments", "<f8", (10,)),
    ]
)
MESH_COUNTS_DTYPE = np.dtype([("n_vertices", "<u4"), ("n_indices", "<u4"), ("n_submeshes", "<u4"), ("reserved", "<u4")])
N_TIMED_STAGES = 10
IMPACT_FRACTURING_CONFIG_DTYPE = np.dtype(
    [("boundary_polar_grid_size", "<u4"), ("boundary_azimuthal_grid_size", "<u4"), ("boundary_angular_jitter", "<f4"), ("boundary_radial_jitter", "<f4"),
     ("max_fragment_count", "<u8"), ("radial_falloff_power", "<f4"), ("angular_falloff_power", "<f4"), ("radial_grid_size", "<u4"),
     ("angular_grid_size", "<u4"), ("max_position_rejections_per_sample", "<u8"), ("seed", "<u8")]
)
FRACTURING_PROPERTIES_DTYPE = np.dtype(
    [("fracturing_force", "<f4"), ("shattering_pressure", "<f4"), ("fragment_scale", "<f4"), ("min_fragment_extent", "<f4"), ("max_fragment_extent", "<f4")]
)
assert IMPACT_FRACTURING_CONFIG_DTYPE.itemsize == 56 and FRACTURING_PROPERTIES_DTYPE.itemsize == 20
SLAB_RESULT_DTYPE = np.dtype(
    [("region_count", "<u4"), ("local_region_count", "<u4"), ("first_local_component", "<u4"), ("reserved", "<u4"), ("moments", "<f8", (10,)),
     ("occupied", "<u4", (12,)), ("mesh", MESH_COUNTS_DTYPE), ("vertex_offset", "<u8"), ("index_offset", "<u8"), ("total_triangles", "<u8"),
     ("stage_ms", "<f4", (10,)), ("reserved2", "<f4", (2,))]
)
# timed slots of a step (include/impact_voxel_hip.h, IVX_N_TIMED_STAGES): the table-sized passes after the derive sweep run as roles of
# four fused launches; 6..9 are unused
STAGE_NAMES = ["sdf_sample", "derive", "post1", "post2", "emit", "assign", "unused6", "unused7", "unused8", "unused9"]
STAGE_SAMPLE, STAGE_DERIVE, STAGE_OCCUPIED, STAGE_REGIONS, STAGE_REMESH, STAGE_INERTIA, STAGE_ALL = 1, 2, 4, 8, 16, 32, 63
STEP_RESULT_DTYPE = np.dtype(
    [
        ("mesh", MESH_COUNTS_DTYPE),
        ("region_count", "<u4"),
        ("occupied", "<u4", (12,)),
        ("reserved", "<u4", (3,)),
        ("moments", MOMENTS_DTYPE),
        ("stage_ms", "<f4", (N_TIMED_STAGES,)),
        ("reserved2", "<f4", (2,)),
    ]
)
assert STEP_RESULT_DTYPE.itemsize == 256
assert CHUNK_INFO_DTYPE.itemsize == 8 and SUBMESH_DTYPE.itemsize == 64
assert MOMENTS_DTYPE.itemsize == 128 and REGION_DESC_DTYPE.itemsize == 128

# rigid bodies / contacts (impact_physics) — reference #[repr(C)] layouts
RIGID_BODY_DTYPE = np.dtype(
    [
        ("mass", "<f4"),
        ("inertia", "<f4", (9,)),       # Matrix3C, column-major
        ("inv_inertia", "<f4", (9,)),
        ("position", "<f4", (3,)),
        ("orientation", "<f4", (4,)),   # x, y, z, w
        ("momentum", "<f4", (3,)),
        ("angular_momentum", "<f4", (3,)),
        ("total_force", "<f4", (3,)),
        ("total_torque", "<f4", (3,)),
    ]
)
KINEMATIC_BODY_DTYPE = np.dtype(
    [("position", "<f4", (3,)), ("orientation", "<f4", (4,)), ("velocity", "<f4", (3,)), ("angular_axis", "<f4", (3,)), ("angular_speed", "<f4")]
)
# `ivx_collidable_query` (ivx_voxel_object_contacts_many): one collidable against one voxel object
COLLIDABLE_QUERY_DTYPE = np.dtype(
    [
        ("mode", "<i4"),
        ("rotation_xyzw", "<f4", (4,)),
        ("translation", "<f4", (3,)),
        ("shape3", "<f4", (3,)),
        ("shape3b", "<f4", (3,)),
        ("shape1", "<f4"),
        ("body_a", "<u4"),
        ("body_b", "<u4"),
        ("collidable_id_a", "<u8"),
        ("collidable_id_b", "<u8"),
        ("response", "<f4", (3,)),
        ("reserved", "<u4"),
    ],
    align=True,
)
# `ivx_mutual_query` (ivx_mutual_voxel_object_contacts_many): one pair of voxel objects
MUTUAL_QUERY_DTYPE = np.dtype(
    [
        ("a", "<u8"),
        ("b", "<u8"),
        ("rotation_a", "<f4", (4,)),
        ("translation_a", "<f4", (3,)),
        ("center_of_mass_a", "<f4", (3,)),
        ("rotation_b", "<f4", (4,)),
        ("translation_b", "<f4", (3,)),
        ("center_of_mass_b", "<f4", (3,)),
        ("collidable_id_a", "<u8"),
        ("collidable_id_b", "<u8"),
        ("body_a", "<u4"),
        ("body_b", "<u4"),
        ("response", "<f4", (3,)),
        ("reserved", "<u4"),
    ],
    align=True,
)
CONTACT_DTYPE = np.dtype(
    [
        ("id", "<u8"),
        ("body_a", "<u4"),
        ("body_b", "<u4"),
        ("position", "<f4", (3,)),
        ("normal", "<f4", (3,)),
        ("depth", "<f4"),
        ("restitution", "<f4"),
        ("static_friction", "<f4"),
        ("dynamic_friction", "<f4"),
        ("flags", "<u4"),
        ("pad", "<u4"),
    ]
)
ABSORB_RESULT_DTYPE = np.dtype([("removed_moments", "<f8", (10,)), ("emptied_voxels", "<u8"), ("touched_chunks", "<u4"), ("removed_chunks", "<u4")])
SOLVER_CONFIG_DTYPE = np.dtype(
    [("n_iterations", "<u4"), ("old_impulse_weight", "<f4"), ("n_positional_correction_iterations", "<u4"), ("positional_correction_factor", "<f4")]
)
PHYSICS_RESULT_DTYPE = np.dtype(
    [("n_contacts", "<u4"), ("n_bodies", "<u4"), ("n_levels", "<u4", (2,)), ("stage_ms", "<f4", (5,)), ("reserved", "<u4", (3,))]
)
PHYSICS_STAGE_NAMES = ["prepare", "pre_solve", "solve", "post_solve", "total"]
KINEMATIC_BIT = 0x80000000
CONTACT_MANIFOLD_START = 1
assert RIGID_BODY_DTYPE.itemsize == 152 and KINEMATIC_BODY_DTYPE.itemsize == 56 and CONTACT_DTYPE.itemsize == 64
# detailed drag (impact_physics/src/force/detailed_drag): `ivx_drag_load` (DragLoad) and the numeric fields of DragLoadMapConfig
DRAG_LOAD_DTYPE = np.dtype([("force", "<f4", (3,)), ("torque", "<f4", (3,))])
DRAG_MAP_CONFIG_DTYPE = np.dtype([("n_direction_samples", "<u4"), ("n_theta_coords", "<u4"), ("smoothness", "<f4"), ("reserved", "<u4")])
assert DRAG_LOAD_DTYPE.itemsize == 24 and DRAG_MAP_CONFIG_DTYPE.itemsize == 16
# chunk culling (csrc/cull.hip): the records of include/impact_voxel_hip.h
CULLING_FRUSTUM_DTYPE = np.dtype([("planes", "<f4", (6, 4)), ("most_inside_corners", "<u4", (6,)), ("apex", "<f4", (3,)), ("instance_idx", "<u4")])
CULL_VIEW_DTYPE = np.dtype([("kind", "<u4"), ("flags", "<u4"), ("planes", "<f4", (6, 4)), ("box_center", "<f4", (3,)), ("box_orientation", "<f4", (4,)),
                            ("box_half_extents", "<f4", (3,)), ("apex_distance", "<f4"), ("reserved", "<u4")])
CULL_PAIR_DTYPE = np.dtype([("rotation", "<f4", (4,)), ("translation", "<f4", (3,)), ("scaling", "<f4"), ("instance_idx", "<u4"), ("flags", "<u4")])
CULL_OBJECT_DTYPE = np.dtype([("first_index_base", "<u4"), ("base_vertex", "<i4")])
DRAW_ARGS_DTYPE = np.dtype([("index_count", "<u4"), ("instance_count", "<u4"), ("first_index", "<u4"), ("first_instance", "<u4")])
DRAW_INDEXED_ARGS_DTYPE = np.dtype([("index_count", "<u4"), ("instance_count", "<u4"), ("first_index", "<u4"), ("base_vertex", "<i4"), ("first_instance", "<u4")])
CULL_REGION_DTYPE = np.dtype([("offset", "<u8"), ("stride", "<u4"), ("n_slots", "<u4")])
CULL_COUNT_DTYPE = np.dtype([("draws", "<u4"), ("indices", "<u4")])
CULL_VIEW_INDEXED, CULL_PAIR_SKIP, CULL_ZEROED, CULL_COMPACTED, CULL_MAX_VIEWS = 1, 1, 0, 1, 64
CULL_PTR_ARGS, CULL_PTR_COUNTS, CULL_PTR_FRUSTA = 0, 1, 2
assert CULLING_FRUSTUM_DTYPE.itemsize == 136 and CULL_VIEW_DTYPE.itemsize == 152 and CULL_PAIR_DTYPE.itemsize == 40 and CULL_OBJECT_DTYPE.itemsize == 8
assert DRAW_ARGS_DTYPE.itemsize == 16 and DRAW_INDEXED_ARGS_DTYPE.itemsize == 20 and CULL_REGION_DTYPE.itemsize == 16 and CULL_COUNT_DTYPE.itemsize == 8
# bounding volumes (csrc/bvol.hip): `ivx_aabb`, `ivx_similarity`, and `ivx_bv_query` — the kind, then the members of its union side by side at
# their offsets (box / sphere / frustum / oriented box all start at byte 4; `words`, the whole payload, comes last so that a field-by-field copy
# of a record ends with the right bytes; bvol.query_array stacks records as bytes)
AABB_DTYPE = np.dtype([("lower", "<f4", (3,)), ("upper", "<f4", (3,))])
SIMILARITY_DTYPE = np.dtype([("rotation", "<f4", (4,)), ("translation", "<f4", (3,)), ("scaling", "<f4")])
BV_QUERY_DTYPE = np.dtype({
    "names": ["kind", "lower", "upper", "center", "radius", "planes", "corners", "axes", "box_center", "half_extents", "words"],
    "formats": ["<u4", ("<f4", (3,)), ("<f4", (3,)), ("<f4", (3,)), "<f4", ("<f4", (6, 4)), ("<u4", (6,)), ("<f4", (3, 3)), ("<f4", (3,)), ("<f4", (3,)), ("<u4", (31,))],
    "offsets": [0, 4, 16, 4, 16, 4, 100, 4, 40, 52, 4],
    "itemsize": 128,
})
BV_DYNAMIC, BV_STATIC, BV_PHANTOM = 0, 1, 2
BV_QUERY_BOX, BV_QUERY_SPHERE, BV_QUERY_FRUSTUM, BV_QUERY_ORIENTED_BOX = 0, 1, 2, 3
BV_ALL_PAIRS, BV_DYNAMIC_PAIRS = 0, 1
BV_PTR_WORLD_BOXES, BV_PTR_PAIRS, BV_PTR_MASKS, BV_PTR_NODES, BV_PTR_LEAF_OBJECTS, BV_PTR_HIT_OFFSETS, BV_PTR_HIT_OBJECTS = 0, 1, 2, 3, 4, 5, 6
BV_MAX_OBJECTS, BV_MAX_QUERIES = 1 << 20, 1024
assert AABB_DTYPE.itemsize == 24 and SIMILARITY_DTYPE.itemsize == 32 and BV_QUERY_DTYPE.itemsize == 128
# the hierarchy over a set (csrc/bvh.hip): `ivx_bv_node`; a child reference with BV_LEAF set names a leaf position, else a node
BV_NODE_DTYPE = np.dtype([("lower", "<f4", (3,)), ("upper", "<f4", (3,)), ("left", "<u4"), ("right", "<u4")])
BV_LEAF = 0x80000000
CW_BROAD_FLAT, CW_BROAD_HIERARCHY = 0, 1
assert BV_NODE_DTYPE.itemsize == 32
# frame instances (csrc/instances.hip): `ivx_fi_instance` (one per object of the context's set), `ivx_fi_view`, `ivx_fi_view_result`
FI_INSTANCE_DTYPE = np.dtype([("model_to_world", SIMILARITY_DTYPE), ("flags", "<u4"), ("entity", "<u4"), ("reserved", "<u4", (2,))])
FI_VIEW_DTYPE = np.dtype([("world_to_view", SIMILARITY_DTYPE), ("query", "<u4"), ("reject_flags", "<u4"), ("exclude_entity", "<u4"), ("and_view", "<u4"),
                          ("instance_base", "<u4"), ("flags", "<u4"), ("point", "<f4", (3,)), ("squared_reach", "<f4")])
FI_VIEW_RESULT_DTYPE = np.dtype([("count", "<u4"), ("world_box", AABB_DTYPE), ("view_box", AABB_DTYPE), ("min_squared_distance", "<f4"), ("max_squared_distance", "<f4")])
FI_ABSENT, FI_HIDDEN, FI_CASTS_NO_SHADOWS, FI_SHADOWS_OFF_BY_DISTANCE, FI_NO_SHADOW_FEATURES, FI_ALL_FLAGS = 1, 2, 4, 8, 16, 31
FI_NONE, FI_VIEW_REACH, FI_VIEW_BOX, FI_MAX_VIEWS = 0xFFFFFFFF, 1, 2, 64
FI_PTR_INSTANCES, FI_PTR_PAIRS, FI_PTR_OFFSETS, FI_PTR_OBJECTS, FI_PTR_TRANSFORMS, FI_PTR_KEPT_MASKS, FI_PTR_RESULTS = 0, 1, 2, 3, 4, 5, 6
assert FI_INSTANCE_DTYPE.itemsize == 48 and FI_VIEW_DTYPE.itemsize == 72 and FI_VIEW_RESULT_DTYPE.itemsize == 60
# primitive collidables (csrc/narrow.hip): `ivx_collidable`, in its body's frame or in world space
COLLIDABLE_DTYPE = np.dtype([("shape", "<u4"), ("kind", "<u4"), ("body", "<u4"), ("reserved", "<u4"), ("id", "<u8"), ("a", "<f4", (3,)), ("b", "<f4", (3,)), ("s", "<f4"),
                             ("response", "<f4", (3,))])
CW_SPHERE, CW_PLANE, CW_CAPSULE, CW_VOXEL_OBJECT = 0, 1, 2, 3
CW_PTR_WORLD_COLLIDABLES, CW_PTR_CONTACTS, CW_PTR_DEFERRED_PAIRS, CW_PTR_FRAME_CONTACTS, CW_PTR_VOXEL_ROWS = 0, 1, 2, 3, 4
assert COLLIDABLE_DTYPE.itemsize == 64
# the collision frame (csrc/narrow.hip k_cw_rows, csrc/voxel_collision_api.hip): `ivx_cw_voxel_object` (what `ivx_cw_set_voxel_objects` attaches to a voxel
# collidable) and `struct ivx_cw_voxel_row` (the dispatch of one deferred pair: an `ivx_collidable_query` or an `ivx_mutual_query` by field copies)
CW_VOXEL_OBJECT_DTYPE = np.dtype([("grid", "<u8"), ("origin_offset", "<f4", (3,)), ("center_of_mass", "<f4", (3,))])
CW_VOXEL_ROW_DTYPE = np.dtype([("generator", "<u4"), ("voxel", "<u4"), ("other", "<u4"), ("reserved", "<u4"), ("collidable_id_a", "<u8"), ("collidable_id_b", "<u8"),
                               ("body_a", "<u4"), ("body_b", "<u4"), ("response", "<f4", (3,)), ("shape1", "<f4"), ("shape3", "<f4", (3,)), ("shape3b", "<f4", (3,)),
                               ("rotation_a", "<f4", (4,)), ("translation_a", "<f4", (3,)), ("center_of_mass_a", "<f4", (3,)),
                               ("rotation_b", "<f4", (4,)), ("translation_b", "<f4", (3,)), ("center_of_mass_b", "<f4", (3,))])
CW_ROW_MUTUAL = 3
assert CW_VOXEL_OBJECT_DTYPE.itemsize == 32 and CW_VOXEL_ROW_DTYPE.itemsize == 160
# motion drivers of kinematic bodies (csrc/motion.hip): `ivx_motion_driver`; `p` holds the reference's setup struct of that kind
MOTION_DRIVER_DTYPE = np.dtype([("kind", "<u4"), ("body", "<u4"), ("p", "<f4", (14,))])
MD_CIRCULAR, MD_CONSTANT_ACCELERATION, MD_HARMONIC, MD_ORBITAL, MD_CONSTANT_ROTATION = 0, 1, 2, 3, 4
assert MOTION_DRIVER_DTYPE.itemsize == 64
# force generators of dynamic bodies (csrc/forces.hip): `ivx_force_generator`; `body_b` is the second body of a spring
FORCE_GENERATOR_DTYPE = np.dtype([("kind", "<u4"), ("body", "<u4"), ("body_b", "<u4"), ("p", "<f4", (13,))])
(FG_CONSTANT_ACCELERATION, FG_LOCAL_FORCE, FG_SPRING_DYNAMIC_DYNAMIC, FG_SPRING_DYNAMIC_KINEMATIC, FG_ALIGNMENT_FIXED,
 FG_ALIGNMENT_GRAVITY) = 0, 1, 2, 3, 4, 5
assert FORCE_GENERATOR_DTYPE.itemsize == 64
# detailed drag inside the force stage (csrc/forces.hip): `ivx_uniform_medium` (UniformMedium), `ivx_drag_generator` (DetailedDragForce on a dynamic
# body, its map a slot of the world's table), `ivx_drag_map_view` (one slot in host memory, for `ivx_fg_apply_host_drag`)
UNIFORM_MEDIUM_DTYPE = np.dtype([("mass_density", "<f4"), ("velocity", "<f4", (3,))])
DRAG_GENERATOR_DTYPE = np.dtype([("body", "<u4"), ("map", "<u4"), ("drag_coefficient", "<f4"), ("scaling", "<f4")])
DRAG_MAP_VIEW_DTYPE = np.dtype([("loads", "<u8"), ("n_theta", "<u4"), ("reserved", "<u4")])
assert UNIFORM_MEDIUM_DTYPE.itemsize == 16 and DRAG_GENERATOR_DTYPE.itemsize == 16 and DRAG_MAP_VIEW_DTYPE.itemsize == 16
# SDF queries (csrc/sdf_query.hip): `ivx_sdf_query_instance` (the subject's node-to-parent similarity, the sphere of the cast in subject space) and
# `ivx_sdf_query_result` (status, steps, translation or rotation quaternion, which Some exit of the cast)
SDF_QUERY_INSTANCE_DTYPE = np.dtype([("subject_to_parent", SIMILARITY_DTYPE), ("sphere_center", "<f4", (3,)), ("sphere_radius", "<f4")])
SDF_QUERY_RESULT_DTYPE = np.dtype([("status", "<u4"), ("steps", "<u4"), ("v", "<f4", (4,)), ("exit", "<u4"), ("reserved", "<u4")])
assert SDF_QUERY_INSTANCE_DTYPE.itemsize == 48 and SDF_QUERY_RESULT_DTYPE.itemsize == 32
SDF_QUERY_MAX_STACK, SDF_QUERY_MAX_ITEMS = 64, 1 << 24
(SQ_OK, SQ_ZERO_GRADIENT, SQ_NO_GRADIENT_DIRECTION, SQ_RAY_MISSES_DOMAIN, SQ_DEGENERATE_DIRECTION, SQ_PENETRATING, SQ_LEFT_INTERVAL, SQ_MAX_STEPS,
 SQ_DEGENERATE_Y_AXIS) = range(9)
SQ_EXIT_CONVERGED, SQ_EXIT_CROSSED = 0, 1

# every symbol include/impact_voxel_hip.h declares
EXPORTED_SYMBOLS = [
    "ivx_init", "ivx_shutdown", "ivx_last_error", "ivx_synchronize", "ivx_stream",
    "ivx_grid_create", "ivx_grid_destroy", "ivx_grid_upload_dense", "ivx_grid_download_dense", "ivx_grid_device_ptr", "ivx_grid_chunk_counts", "ivx_grid_stage_counters",
    "ivx_sdf_compile", "ivx_sdf_grid_shape", "ivx_sdf_sample",
    "ivx_derive_state", "ivx_occupied_ranges",
    "ivx_remesh", "ivx_mesh_download", "ivx_mesh_device_ptr",
    "ivx_inertia",
    "ivx_label_regions", "ivx_region_labels_download", "ivx_regions_describe", "ivx_split_off_smallest_region", "ivx_split_off_all", "ivx_clip_polyhedron", "ivx_copy_polyhedra", "ivx_mesh_sync", "ivx_mesh_export", "ivx_mesh_generation", "ivx_mesh_import_open", "ivx_mesh_import_close", "ivx_mesh_modifications", "ivx_mesh_report_synchronized", "ivx_absorb_sphere", "ivx_absorb_capsule", "ivx_absorb_mutual", "ivx_absorb_sphere_enqueue", "ivx_absorb_capsule_enqueue", "ivx_absorb_collect", "ivx_grid_set_early_mesh_needs", "ivx_mesh_sync_enqueue", "ivx_mesh_sync_collect",
    "ivx_many_begin", "ivx_many_flush", "ivx_many_stats", "ivx_voxel_step_many", "ivx_absorb_sphere_many", "ivx_absorb_capsule_many", "ivx_mesh_sync_many", "ivx_offset_reference_point", "ivx_apply_updated_inertial_properties", "ivx_extracted_object_dynamics", "ivx_handle_voxel_object_after_removing_voxels", "ivx_sphere_voxel_object_contacts", "ivx_plane_voxel_object_contacts", "ivx_capsule_voxel_object_contacts", "ivx_voxel_object_contacts_many", "ivx_collision_probes_recompute", "ivx_collision_probes_sync", "ivx_collision_probes_sync_many", "ivx_collision_probes_download", "ivx_mutual_voxel_object_contacts", "ivx_mutual_voxel_object_contacts_many",
    "ivx_grid_set_sdf_program", "ivx_grid_set_densities", "ivx_grid_set_voxel_type_noise", "ivx_voxel_step", "ivx_voxel_step_enqueue", "ivx_voxel_step_collect", "ivx_grid_set_stage_timing", "ivx_debug_stage_ticks", "ivx_grid_set_sample_ahead",
    "ivx_halo_pack_enqueue", "ivx_halo_unpack_enqueue", "ivx_halo_pack_both_enqueue", "ivx_region_face_labels_enqueue", "ivx_region_face_pairs_enqueue",
    "ivx_step_record_words", "ivx_step_record_enqueue", "ivx_slab_remesh_enqueue",
    "ivx_halo_bytes", "ivx_halo_pack", "ivx_halo_unpack", "ivx_halo_clear",
    "ivx_region_face_bytes", "ivx_region_face_labels", "ivx_region_face_pairs",
    "ivx_world_create", "ivx_world_destroy", "ivx_world_set_bodies", "ivx_world_get_bodies", "ivx_world_set_contacts",
    "ivx_world_set_spherical_joints", "ivx_world_step", "ivx_world_step_enqueue", "ivx_world_prepare", "ivx_world_advance_momenta", "ivx_world_solve", "ivx_world_advance_configurations",
    "ivx_impact_fracturing_config_default", "ivx_generate_impact_fracture_points", "ivx_delaunay_construct", "ivx_delaunay_destroy", "ivx_delaunay_counts",
    "ivx_delaunay_download", "ivx_delaunay_aabb", "ivx_delaunay_displace_vertices", "ivx_delaunay_boundary_face_planes", "ivx_voronoi_polyhedron", "ivx_voronoi_bounded_aabb",
    "ivx_comm_unique_id", "ivx_comm_init", "ivx_comm_init_local", "ivx_comm_init_ipc", "ivx_comm_info", "ivx_comm_set_local_copies", "ivx_comm_selftest", "ivx_selftest_mesher_division", "ivx_noise_eval", "ivx_voxel_types_eval", "ivx_sampler_plan", "ivx_comm_destroy", "ivx_slab_create", "ivx_slab_destroy",
    "ivx_slabs_step_enqueue", "ivx_slabs_step_collect", "ivx_slab_region_map",
    "ivx_world_set_solver_groups", "ivx_world_solver_info", "ivx_world_contact_state",
    "ivx_drag_map_config_default", "ivx_drag_directions", "ivx_drag_map_indices", "ivx_drag_force_and_torque",
    "ivx_drag_loads_triangles", "ivx_drag_loads", "ivx_drag_load_map_from_samples", "ivx_drag_load_map",
    "ivx_culling_frustum_from_view", "ivx_cull_frusta", "ivx_cull_submesh_tables", "ivx_cull_submesh_tables_frusta", "ivx_cull_many", "ivx_cull_many_enqueue",
    "ivx_cull_collect", "ivx_cull_many_frusta", "ivx_cull_download", "ivx_cull_device_ptr",
    "ivx_bv_world_aabb", "ivx_bv_frustum_query", "ivx_grid_model_aabb", "ivx_bv_set", "ivx_bv_set_grids", "ivx_bv_download", "ivx_bv_pairs", "ivx_bv_queries",
    "ivx_bv_device_ptr",
    "ivx_bv_morton_key", "ivx_bv_hierarchy_host", "ivx_bv_build_hierarchy", "ivx_bv_hierarchy_download", "ivx_bv_pairs_hierarchy", "ivx_cw_set_broad_phase",
    "ivx_bv_queries_hierarchy", "ivx_bv_queries_hierarchy_host", "ivx_bv_query_skips_boxes", "ivx_bv_query_lists",
    "ivx_fi_set_instances", "ivx_fi_views", "ivx_fi_download", "ivx_fi_device_ptr", "ivx_fi_views_host", "ivx_cull_many_resident",
    "ivx_cw_transform", "ivx_cw_contact", "ivx_cw_set_collidables", "ivx_cw_synchronize", "ivx_cw_download", "ivx_cw_collide", "ivx_cw_device_ptr",
    "ivx_cw_to_object_space", "ivx_cw_voxel_row", "ivx_cw_set_voxel_objects", "ivx_cw_collide_frame", "ivx_cw_rows_download",
    "ivx_world_set_motion_drivers", "ivx_world_set_time", "ivx_world_time", "ivx_world_apply_motion", "ivx_md_eval", "ivx_md_apply_host",
    "ivx_world_set_force_generators", "ivx_world_set_dynamic_gravity", "ivx_world_apply_forces", "ivx_world_gravity_loads", "ivx_fg_apply_host",
    "ivx_world_set_medium", "ivx_world_medium", "ivx_world_set_drag_map", "ivx_world_set_drag_map_from_grid", "ivx_world_drag_map_download",
    "ivx_world_set_detailed_drag", "ivx_fg_apply_host_drag",
    "ivx_sdf_query_create", "ivx_sdf_query_destroy", "ivx_sdf_query_points", "ivx_sdf_query_closest", "ivx_sdf_query_spherecast", "ivx_sdf_query_rotation",
]


MESH_EXPORT_DTYPE = np.dtype([("ipc_handle", "u1", (64,)), ("dmabuf_fd", "<i4"), ("element_bytes", "<u4"), ("bytes", "<u8"), ("capacity_bytes", "<u8"),
                              ("generation", "<u8"), ("device_ptr", "<u8"), ("dmabuf_offset", "<u8"), ("dmabuf_bytes", "<u8")])

EXTRACTED_OBJECT_DTYPE = np.dtype(
    [
        ("grid", "<u8"),
        ("origin_offset_in_parent", "<u4", (3,)),
        ("reserved", "<u4"),
        ("body", RIGID_BODY_DTYPE),
        ("moments", "<f8", (10,)),
        ("local_center_of_mass", "<f4", (3,)),
        ("reserved2", "<f4"),
    ]
)
assert EXTRACTED_OBJECT_DTYPE.itemsize == 272


def extra_struct_sizes():
    """name -> (dtype, size the header documents) for the structs not asserted above"""
    return {
        "ivx_rigid_body": (RIGID_BODY_DTYPE, 152), "ivx_kinematic_body": (KINEMATIC_BODY_DTYPE, 56), "ivx_contact": (CONTACT_DTYPE, 64),
        "ivx_solver_config": (SOLVER_CONFIG_DTYPE, 16), "ivx_physics_result": (PHYSICS_RESULT_DTYPE, 48),
        "ivx_absorb_result": (ABSORB_RESULT_DTYPE, 96), "ivx_extracted_object": (EXTRACTED_OBJECT_DTYPE, 272),
        "ivx_drag_load": (DRAG_LOAD_DTYPE, 24), "ivx_drag_map_config": (DRAG_MAP_CONFIG_DTYPE, 16),
        "ivx_culling_frustum": (CULLING_FRUSTUM_DTYPE, 136), "ivx_cull_view": (CULL_VIEW_DTYPE, 152), "ivx_cull_pair": (CULL_PAIR_DTYPE, 40),
        "ivx_cull_object": (CULL_OBJECT_DTYPE, 8), "ivx_draw_args": (DRAW_ARGS_DTYPE, 16), "ivx_draw_indexed_args": (DRAW_INDEXED_ARGS_DTYPE, 20),
        "ivx_cull_region": (CULL_REGION_DTYPE, 16), "ivx_cull_count": (CULL_COUNT_DTYPE, 8),
        "ivx_aabb": (AABB_DTYPE, 24), "ivx_similarity": (SIMILARITY_DTYPE, 32), "ivx_bv_query": (BV_QUERY_DTYPE, 128), "ivx_bv_node": (BV_NODE_DTYPE, 32),
        "ivx_fi_instance": (FI_INSTANCE_DTYPE, 48), "ivx_fi_view": (FI_VIEW_DTYPE, 72), "ivx_fi_view_result": (FI_VIEW_RESULT_DTYPE, 60),
        "ivx_collidable": (COLLIDABLE_DTYPE, 64), "ivx_cw_voxel_object": (CW_VOXEL_OBJECT_DTYPE, 32), "ivx_cw_voxel_row": (CW_VOXEL_ROW_DTYPE, 160),
        "ivx_motion_driver": (MOTION_DRIVER_DTYPE, 64),
        "ivx_force_generator": (FORCE_GENERATOR_DTYPE, 64),
        "ivx_uniform_medium": (UNIFORM_MEDIUM_DTYPE, 16), "ivx_drag_generator": (DRAG_GENERATOR_DTYPE, 16), "ivx_drag_map_view": (DRAG_MAP_VIEW_DTYPE, 16),
        "ivx_sdf_query_instance": (SDF_QUERY_INSTANCE_DTYPE, 48), "ivx_sdf_query_result": (SDF_QUERY_RESULT_DTYPE, 32),
    }


# ivx_sampler_plan (developer export): word counts of its two arrays, the header's IVX_SAMPLER_PLAN_*_WORDS
SAMPLER_PLAN_IN_WORDS, SAMPLER_PLAN_OUT_WORDS = 19, 48


class IvxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ivx error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load the shared library (fails loudly when it is missing: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch (ROCm wheel) bundles its own HIP runtime; two runtimes in one process cannot both own the GPU
    # ("No HIP GPUs are available" in whichever initialises second). Importing torch first makes this
    # library bind to the runtime torch already loaded, so device buffers and streams can be shared.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise IvxError(IVX_ERR_HIP, f"{LIB_PATH} not found — run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    vp, u32, i32, sz, f32 = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t, C.c_float
    sig = {
        "ivx_init": (i32, [i32, vp, C.POINTER(vp)]),
        "ivx_shutdown": (None, [vp]),
        "ivx_last_error": (C.c_char_p, []),
        "ivx_synchronize": (i32, [vp]),
        "ivx_stream": (vp, [vp]),
        "ivx_grid_create": (i32, [vp, vp, f32, u32, u32, C.POINTER(vp)]),
        "ivx_grid_destroy": (None, [vp]),
        "ivx_grid_upload_dense": (i32, [vp, vp, vp, sz]),
        "ivx_grid_download_dense": (i32, [vp, vp, vp, vp, vp, vp, sz]),
        "ivx_grid_device_ptr": (vp, [vp, i32]),
        "ivx_grid_chunk_counts": (i32, [vp, vp]),
        "ivx_grid_stage_counters": (i32, [vp, vp]),
        "ivx_sdf_compile": (i32, [vp, sz, u32, vp, sz, C.POINTER(sz), vp, C.POINTER(u32)]),
        "ivx_sdf_grid_shape": (i32, [vp, vp, vp]),
        "ivx_noise_eval": (i32, [vp, i32, vp, vp, sz, vp]),
        "ivx_voxel_types_eval": (i32, [vp, u32, f32, f32, u32, vp, vp]),
        "ivx_sampler_plan": (i32, [vp, vp]),
        "ivx_sdf_sample": (i32, [vp, vp, sz, u32, vp, vp, C.c_uint8]),
        "ivx_derive_state": (i32, [vp]),
        "ivx_occupied_ranges": (i32, [vp, vp]),
        "ivx_remesh": (i32, [vp, vp]),
        "ivx_mesh_download": (i32, [vp, vp, vp, vp, vp, vp]),
        "ivx_mesh_device_ptr": (vp, [vp, i32]),
        "ivx_inertia": (i32, [vp, vp, vp]),
        "ivx_label_regions": (i32, [vp, C.POINTER(u32)]),
        "ivx_region_labels_download": (i32, [vp, vp, sz]),
        "ivx_regions_describe": (i32, [vp, vp, vp, sz, C.POINTER(sz)]),
        "ivx_split_off_smallest_region": (i32, [vp, C.POINTER(vp), vp, C.POINTER(i32), vp]),
        "ivx_split_off_all": (i32, [vp, C.c_size_t, vp, vp, vp, vp, vp]),
        "ivx_clip_polyhedron": (i32, [vp, vp, sz, vp, i32, C.POINTER(vp), vp, C.POINTER(i32)]),
        "ivx_copy_polyhedra": (i32, [vp, vp, vp, vp, sz, vp, vp, vp]),
        "ivx_grid_set_sdf_program": (i32, [vp, vp, sz, u32, vp, vp, C.c_uint8]),
        "ivx_grid_set_densities": (i32, [vp, vp]),
        "ivx_grid_set_voxel_type_noise": (i32, [vp, u32, f32, f32, u32]),
        "ivx_voxel_step": (i32, [vp, u32, vp]),
        "ivx_voxel_step_enqueue": (i32, [vp, u32]),
        "ivx_voxel_step_collect": (i32, [vp, vp]),
        "ivx_grid_set_stage_timing": (i32, [vp, u32]),
        "ivx_debug_stage_ticks": (i32, [vp, vp, vp]),
        "ivx_grid_set_sample_ahead": (i32, [vp, i32]),
        "ivx_halo_pack_enqueue": (i32, [vp, i32, vp]),
        "ivx_halo_unpack_enqueue": (i32, [vp, i32, vp]),
        "ivx_halo_pack_both_enqueue": (i32, [vp, vp, vp, i32]),
        "ivx_region_face_labels_enqueue": (i32, [vp, i32, vp]),
        "ivx_region_face_pairs_enqueue": (i32, [vp, i32, vp]),
        "ivx_step_record_words": (sz, []),
        "ivx_step_record_enqueue": (i32, [vp, vp]),
        "ivx_slab_remesh_enqueue": (i32, [vp, vp, vp]),
        "ivx_halo_bytes": (sz, [vp]),
        "ivx_halo_pack": (i32, [vp, i32, vp]),
        "ivx_halo_unpack": (i32, [vp, i32, vp]),
        "ivx_halo_clear": (i32, [vp, i32]),
        "ivx_region_face_bytes": (sz, [vp]),
        "ivx_region_face_labels": (i32, [vp, i32, vp]),
        "ivx_region_face_pairs": (i32, [vp, i32, vp, vp, sz, C.POINTER(sz)]),
        "ivx_world_create": (i32, [vp, vp, C.POINTER(vp)]),
        "ivx_world_destroy": (None, [vp]),
        "ivx_world_set_bodies": (i32, [vp, vp, sz, vp, sz]),
        "ivx_world_get_bodies": (i32, [vp, vp, vp]),
        "ivx_world_set_contacts": (i32, [vp, vp, sz, C.POINTER(sz)]),
        "ivx_mesh_sync": (i32, [vp, vp, vp]),
        "ivx_mesh_modifications": (i32, [vp, vp, sz, C.POINTER(sz), C.POINTER(i32)]),
        "ivx_mesh_report_synchronized": (i32, [vp]),
        "ivx_absorb_sphere": (i32, [vp, vp, f32, f32, vp, vp, vp, vp]),
        "ivx_absorb_sphere_enqueue": (i32, [vp, vp, f32, f32, vp]),
        "ivx_absorb_capsule_enqueue": (i32, [vp, vp, vp, f32, f32, vp]),
        "ivx_absorb_collect": (i32, [vp, vp, vp, vp]),
        "ivx_many_begin": (i32, [vp]),
        "ivx_many_flush": (i32, [vp]),
        "ivx_many_stats": (i32, [vp, vp]),
        "ivx_voxel_step_many": (i32, [vp, sz, u32, vp]),
        "ivx_absorb_sphere_many": (i32, [vp, sz, vp, vp, vp, vp, vp, vp]),
        "ivx_absorb_capsule_many": (i32, [vp, sz, vp, vp, vp, vp, vp, vp, vp]),
        "ivx_mesh_sync_many": (i32, [vp, sz, vp, vp]),
        "ivx_mesh_sync_enqueue": (i32, [vp, vp]),
        "ivx_grid_set_early_mesh_needs": (i32, [vp, i32]),
        "ivx_mesh_sync_collect": (i32, [vp, vp]),
        "ivx_offset_reference_point": (i32, [vp, vp]),
        "ivx_apply_updated_inertial_properties": (i32, [vp, vp, vp, i32, vp]),
        "ivx_extracted_object_dynamics": (i32, [vp, vp, f32, vp, vp, vp, vp]),
        "ivx_handle_voxel_object_after_removing_voxels": (i32, [vp, vp, vp, vp, vp, i32, vp, sz, C.POINTER(sz), C.POINTER(i32), vp]),
        "ivx_absorb_mutual": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp]),
        "ivx_absorb_capsule": (i32, [vp, vp, vp, f32, f32, vp, vp, vp, vp]),
        "ivx_sphere_voxel_object_contacts": (i32, [vp, vp, vp, vp, f32, C.c_uint64, C.c_uint64, u32, u32, vp, vp, sz, C.POINTER(sz)]),
        "ivx_plane_voxel_object_contacts": (i32, [vp, vp, vp, vp, f32, C.c_uint64, C.c_uint64, u32, u32, vp, vp, sz, C.POINTER(sz)]),
        "ivx_collision_probes_recompute": (i32, [vp, C.POINTER(sz)]),
        "ivx_collision_probes_sync": (i32, [vp, vp, C.POINTER(sz)]),
        "ivx_collision_probes_sync_many": (i32, [vp, C.c_size_t, vp, vp]),
        "ivx_collision_probes_download": (i32, [vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz)]),
        "ivx_mutual_voxel_object_contacts": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, u32, u32, vp, vp, sz, C.POINTER(sz)]),
        "ivx_mutual_voxel_object_contacts_many": (i32, [vp, C.c_size_t, vp, C.c_size_t, vp]),
        "ivx_capsule_voxel_object_contacts": (i32, [vp, vp, vp, vp, vp, f32, C.c_uint64, C.c_uint64, u32, u32, vp, vp, sz, C.POINTER(sz)]),
        "ivx_voxel_object_contacts_many": (i32, [vp, C.c_size_t, vp, vp, C.c_size_t, vp]),
        "ivx_world_step": (i32, [vp, f32, vp]),
        "ivx_world_step_enqueue": (i32, [vp, f32]),
        "ivx_world_set_spherical_joints": (i32, [vp, vp, sz]),
        "ivx_world_prepare": (i32, [vp]),
        "ivx_world_advance_momenta": (i32, [vp, f32]),
        "ivx_world_solve": (i32, [vp]),
        "ivx_world_advance_configurations": (i32, [vp, f32]),
        "ivx_world_contact_state": (i32, [vp, vp, vp, sz, C.POINTER(sz)]),
        "ivx_impact_fracturing_config_default": (None, [vp]),
        "ivx_generate_impact_fracture_points": (i32, [vp, vp, f32, vp, vp, vp, vp, vp, f32, vp, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz)]),
        "ivx_delaunay_construct": (i32, [vp, sz, C.POINTER(vp)]),
        "ivx_delaunay_destroy": (None, [vp]),
        "ivx_delaunay_counts": (i32, [vp, vp]),
        "ivx_delaunay_download": (i32, [vp, vp, vp, vp]),
        "ivx_delaunay_aabb": (i32, [vp, vp]),
        "ivx_delaunay_displace_vertices": (i32, [vp, vp]),
        "ivx_delaunay_boundary_face_planes": (i32, [vp, vp, sz, C.POINTER(sz)]),
        "ivx_voronoi_polyhedron": (i32, [vp, u32, vp, sz, vp, sz, vp, sz, vp]),
        "ivx_voronoi_bounded_aabb": (i32, [vp, sz, vp, sz, vp, vp, C.POINTER(i32)]),
        "ivx_comm_unique_id": (i32, [vp]),
        "ivx_comm_init": (i32, [vp, i32, i32, vp, C.POINTER(vp)]),
        "ivx_comm_init_local": (i32, [vp, i32, C.POINTER(vp)]),
        "ivx_comm_init_ipc": (i32, [vp, i32, i32, C.c_char_p, C.POINTER(vp)]),
        "ivx_mesh_export": (i32, [vp, i32, vp]),
        "ivx_mesh_generation": (i32, [vp, C.POINTER(C.c_uint64)]),
        "ivx_mesh_import_open": (i32, [vp, i32, C.POINTER(vp)]),
        "ivx_mesh_import_close": (i32, [vp]),
        "ivx_comm_info": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "ivx_comm_set_local_copies": (i32, [vp, i32]),
        "ivx_comm_selftest": (i32, [vp]),
        "ivx_selftest_mesher_division": (i32, [vp, C.POINTER(u32)]),
        "ivx_comm_destroy": (None, [vp]),
        "ivx_slab_create": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "ivx_slab_destroy": (None, [vp]),
        "ivx_slabs_step_enqueue": (i32, [vp, sz]),
        "ivx_slabs_step_collect": (i32, [vp, sz, vp]),
        "ivx_slab_region_map": (i32, [vp, i32, vp, sz, C.POINTER(sz)]),
        "ivx_world_set_solver_groups": (i32, [vp, u32]),
        "ivx_world_solver_info": (i32, [vp, vp]),
        "ivx_drag_map_config_default": (None, [vp]),
        "ivx_drag_directions": (i32, [sz, vp]),
        "ivx_drag_map_indices": (i32, [u32, f32, f32, C.POINTER(u32), C.POINTER(u32)]),
        "ivx_drag_force_and_torque": (i32, [vp, u32, vp, vp, f32, f32, f32]),
        "ivx_drag_loads_triangles": (i32, [vp, vp, sz, vp, sz, vp, vp, sz, vp]),
        "ivx_drag_loads": (i32, [vp, vp, vp, sz, vp]),
        "ivx_drag_load_map_from_samples": (i32, [vp, vp, vp, sz, u32, f32, vp]),
        "ivx_drag_load_map": (i32, [vp, vp, vp, vp]),
        "ivx_culling_frustum_from_view": (i32, [vp, vp, f32, vp]),
        "ivx_cull_frusta": (i32, [vp, vp, sz, vp, vp, sz, vp]),
        "ivx_cull_submesh_tables": (i32, [vp, vp, vp, sz, vp, vp, vp, sz, vp, u32, vp, vp]),
        "ivx_cull_submesh_tables_frusta": (i32, [vp, vp, vp, sz, vp, vp, vp, vp, sz, u32, vp, vp]),
        "ivx_cull_many": (i32, [vp, sz, vp, vp, sz, vp, u32, vp, vp]),
        "ivx_cull_many_enqueue": (i32, [vp, sz, vp, vp, sz, vp, u32, vp]),
        "ivx_cull_collect": (i32, [vp, vp, sz]),
        "ivx_cull_many_frusta": (i32, [vp, sz, vp, vp, vp, vp, sz, u32, vp, vp]),
        "ivx_cull_download": (i32, [vp, u32, vp, sz, vp, vp, sz]),
        "ivx_cull_device_ptr": (vp, [vp, i32]),
        "ivx_bv_world_aabb": (i32, [vp, vp, vp]),
        "ivx_bv_frustum_query": (i32, [vp, vp]),
        "ivx_grid_model_aabb": (i32, [vp, vp]),
        "ivx_bv_set": (i32, [vp, vp, vp, vp, sz]),
        "ivx_bv_set_grids": (i32, [vp, sz, vp, vp]),
        "ivx_bv_download": (i32, [vp, vp, sz, vp]),
        "ivx_bv_pairs": (i32, [vp, u32, vp, sz, C.POINTER(sz)]),
        "ivx_bv_queries": (i32, [vp, vp, sz, vp, vp]),
        "ivx_bv_device_ptr": (vp, [vp, i32]),
        "ivx_bv_morton_key": (i32, [vp, vp, u32, C.POINTER(C.c_uint64)]),
        "ivx_bv_hierarchy_host": (i32, [vp, sz, vp, vp, vp]),
        "ivx_bv_build_hierarchy": (i32, [vp]),
        "ivx_bv_hierarchy_download": (i32, [vp, vp, sz, vp, sz, C.POINTER(sz)]),
        "ivx_bv_pairs_hierarchy": (i32, [vp, u32, vp, sz, C.POINTER(sz)]),
        "ivx_bv_queries_hierarchy": (i32, [vp, vp, sz, vp, vp]),
        "ivx_bv_queries_hierarchy_host": (i32, [vp, sz, vp, vp, vp, sz, vp, vp]),
        "ivx_bv_query_skips_boxes": (i32, [vp, sz, vp, sz, vp]),
        "ivx_bv_query_lists": (i32, [vp, vp, vp, sz, C.POINTER(sz)]),
        "ivx_cw_set_broad_phase": (i32, [vp, u32]),
        "ivx_fi_set_instances": (i32, [vp, vp, sz]),
        "ivx_fi_views": (i32, [vp, vp, sz, vp]),
        "ivx_fi_download": (i32, [vp, vp, sz, vp, sz, vp, vp, sz, vp, sz, C.POINTER(sz)]),
        "ivx_fi_device_ptr": (vp, [vp, i32]),
        "ivx_fi_views_host": (i32, [vp, sz, vp, vp, sz, vp, sz, vp, sz, vp, vp, vp, vp, sz, vp, vp]),
        "ivx_cull_many_resident": (i32, [vp, sz, vp, vp, vp, sz, u32, vp]),
        "ivx_cw_transform": (i32, [vp, vp, vp, vp, vp]),
        "ivx_cw_contact": (i32, [vp, vp, vp, C.POINTER(i32)]),
        "ivx_cw_set_collidables": (i32, [vp, vp, sz]),
        "ivx_cw_synchronize": (i32, [vp]),
        "ivx_cw_download": (i32, [vp, vp, sz]),
        "ivx_cw_collide": (i32, [vp, u32, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz)]),
        "ivx_cw_device_ptr": (vp, [vp, i32]),
        "ivx_cw_to_object_space": (i32, [vp, vp, vp, vp, vp]),
        "ivx_cw_voxel_row": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "ivx_cw_set_voxel_objects": (i32, [vp, vp, vp, sz]),
        "ivx_cw_collide_frame": (i32, [vp, u32, vp, sz, C.POINTER(sz), C.POINTER(sz), vp, vp, sz, C.POINTER(sz)]),
        "ivx_cw_rows_download": (i32, [vp, vp, sz, C.POINTER(sz)]),
        "ivx_world_set_motion_drivers": (i32, [vp, vp, sz]),
        "ivx_world_set_time": (i32, [vp, f32]),
        "ivx_world_time": (i32, [vp, C.POINTER(f32)]),
        "ivx_world_apply_motion": (i32, [vp, f32]),
        "ivx_md_eval": (i32, [vp, f32, vp]),
        "ivx_md_apply_host": (i32, [vp, sz, vp, sz, f32]),
        "ivx_world_set_force_generators": (i32, [vp, vp, sz]),
        "ivx_world_set_dynamic_gravity": (i32, [vp, vp, sz, f32]),
        "ivx_world_apply_forces": (i32, [vp]),
        "ivx_world_gravity_loads": (i32, [vp, vp, sz]),
        "ivx_fg_apply_host": (i32, [vp, sz, vp, sz, f32, vp, sz, vp, sz, vp]),
        "ivx_world_set_medium": (i32, [vp, vp]),
        "ivx_world_medium": (i32, [vp, vp]),
        "ivx_world_set_drag_map": (i32, [vp, u32, vp, u32]),
        "ivx_world_set_drag_map_from_grid": (i32, [vp, u32, vp, vp, vp]),
        "ivx_world_drag_map_download": (i32, [vp, u32, vp, sz, C.POINTER(u32)]),
        "ivx_world_set_detailed_drag": (i32, [vp, vp, sz]),
        "ivx_fg_apply_host_drag": (i32, [vp, sz, vp, sz, f32, vp, sz, vp, sz, vp, vp, sz, vp, sz, vp]),
        "ivx_sdf_query_create": (i32, [vp, vp, sz, u32, vp, C.POINTER(vp)]),
        "ivx_sdf_query_destroy": (None, [vp]),
        "ivx_sdf_query_points": (i32, [vp, i32, vp, sz, vp]),
        "ivx_sdf_query_closest": (i32, [vp, vp, vp, sz, u32, f32, vp]),
        "ivx_sdf_query_spherecast": (i32, [vp, vp, vp, sz, vp, u32, f32, f32, vp]),
        "ivx_sdf_query_rotation": (i32, [vp, vp, vp, sz, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(code):
    if code != IVX_OK:
        raise IvxError(code, lib().ivx_last_error().decode("utf-8", "replace"))


def ptr(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)
