"""softbodyunity_amd — MI355X-native soft-body solver behind the Unity Softbody component API.

Product package: HIP kernels + C-ABI plugin (csrc/, libsoftbody_mi355x.so), the ctypes twin of the C#
P/Invoke layer (native.py), the Softbody component mirror (softbody.py) and the synthetic mesh
generators (mesh.py). The CPU oracle lives in /oracle and is never imported from here.
"""
from .mesh import (SoftbodyMesh, bunny_surrogate, embed_vertices, from_tet_mesh, from_triangle_mesh, jelly_cube,  # noqa: F401
                   read_gmsh, read_tetgen, signed_distance_grid)
from .native import distance_field, distance_field_pose, heightfield  # noqa: F401
from .softbody import (CLOSEST_HIT, IMPULSE, Softbody, SoftbodyGroup, box_collider, capsule_collider, comm_unique_id,  # noqa: F401
                       impulse_explosion, impulse_hits, impulse_particles, make_closest_queries, make_placement, make_surface_force,
                       placement_from_rotation, sphere_collider)
