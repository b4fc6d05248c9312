"""Build libninpol_amd.so in-tree: hand-written HIP for gfx950 + the host grid builder.

`python -m ninpol_amd.build` (or __graft_entry__.build()).  hipcc cross-compiles without a GPU.
The shared object lives next to this file so it travels with the tree to the GPU box.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libninpol_amd.so")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = "gfx950"

# (source, compiler, extra flags)
UNITS = [
    # host connectivity: g++ + libgomp; no FMA contraction (float32 normals must match the reference)
    ("grid_host.cpp", "g++", ["-fopenmp", "-ffp-contract=off"]),
    # native table packing; diff_mag must be the reference's value bit for bit: no contraction either
    ("pack_host.cpp", "g++", ["-fopenmp", "-ffp-contract=off"]),
    # IDW / LS: contraction off so results are the reference's bit for bit
    ("kernels_idw_ls.hip", "hipcc", ["-ffp-contract=off"]),
    ("kernels_gls.hip", "hipcc", []),
    ("kernels_gls_block.hip", "hipcc", []),
    # no atomic optimizer: it turns the work-queue atomicAdd into mbcnt + readfirstlane of the returned value right
    # behind the atomic, i.e. a full round-trip wait at the top of every pass; left alone the value is first read at
    # the end of the pass (kernels_gls_hex8mf.hip, grab_issue / grab_value)
    ("kernels_gls_hex8mf.hip", "hipcc", ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None"]),
    ("kernels_gls_mfw.hip", "hipcc", []),
    ("kernels_gls_mfx.hip", "hipcc", []),
    ("kernels_gls_mfg.hip", "hipcc", []),
    ("kernels_gls_quad4.hip", "hipcc", []),
    # the GLS weights differentiated with respect to the permeability: a dense QR per node kept for two solves, and the gather
    ("kernels_gls_adjoint.hip", "hipcc", []),
    # the adjoint in the node coordinates, from the records of the adjoint kernel's coordinate mode to the vertices: three gathers;
    # and the same geometry read forwards for the tangent in the coordinates: a direction of the nodes to cells and faces
    ("kernels_gls_shape.hip", "hipcc", []),
    # the Jacobian that one adjoint launch leaves in a contribution buffer, applied: J . dK node-major, J^T . v cell-major
    ("kernels_gls_jacobian.hip", "hipcc", []),
    # the same Jacobian in M = 1, 3 or 6 parameters per cell: R [nnz_esup][M] streamed, 8 M bytes per entry instead of 80
    ("kernels_gls_jacobian_reduced.hip", "hipcc", []),
    # the Jacobian in the node coordinates that one launch of the adjoint kernel's coordinate mode leaves in three record buffers,
    # applied through the mesh geometry: J . dX node-major, J^T . v as the shape adjoint's three gathers with a factor
    ("kernels_gls_shape_jacobian.hip", "hipcc", []),
    # the same records assembled into a block-CSR matrix: a symbolic pass per object (the column set of every row), a numeric pass per
    # linearisation
    ("kernels_gls_shape_assemble.hip", "hipcc", []),
    # what follows the corner gradients of the adjoint kernel's gradient mode: the fluxes -K g and the nodal mean, streamed; no contraction,
    # so that the host gets the same bits from the stated expression
    ("kernels_gls_gradient.hip", "hipcc", ["-ffp-contract=off"]),
    # the corner-gradient operator the adjoint kernel's gradient mode leaves, applied: G . u per entry of esup, G^T . v per column and then
    # per cell; no contraction, so that the host gets the same bits from the stated sums
    ("kernels_gls_gradop.hip", "hipcc", ["-ffp-contract=off"]),
    ("kernels_csr.hip", "hipcc", []),
    # an incremental interpolate(): the dirty rows counted and packed on the device, patched into the caller's matrix on the host
    ("csr_dirty.hip", "hipcc", []),
    ("csr_patch.cpp", "g++", ["-fopenmp"]),
    # device-side grid build: no contraction, like grid_host.cpp (float32 normals must match the reference)
    ("grid_device.hip", "hipcc", ["-ffp-contract=off"]),
    # geometry refresh of a moving mesh: the same arithmetic as grid_device.hip's geometry kernels, the same flag
    ("grid_update.hip", "hipcc", ["-ffp-contract=off"]),
    # local mesh motion: the cells and faces around the moved nodes get grid_update.hip's arithmetic (geom_math.hpp) under the same flag
    ("grid_scatter.hip", "hipcc", ["-ffp-contract=off"]),
    # permeability from device memory: diff_mag must be pack_host.cpp's value bit for bit, so no contraction here either
    ("fields_update.hip", "hipcc", ["-ffp-contract=off"]),
    # local permeability updates: the scatter's diff_mag is the same expression under the same flag
    ("fields_scatter.hip", "hipcc", ["-ffp-contract=off"]),
    # Neumann flags from device memory: integer work on bytes, one float64 -> integer cast; nothing to contract
    ("flags_update.hip", "hipcc", []),
    # a kept Jacobian follows local updates: the dirty set binned by adjoint bin, the cotangent for the listed rows, marks without an
    # update; integer work and copies, nothing to contract (the adjoint kernel itself stays in its own unit, launched on these lists)
    ("jacobian_dirty.hip", "hipcc", []),
    # the C ABI's host code by area (abi_internal.hpp is what they share); only abi_plan.hip has a kernel, the locality keys
    ("abi_grid.hip", "hipcc", ["-Wno-unknown-pragmas"]),
    ("abi_plan.hip", "hipcc", ["-Wno-unknown-pragmas"]),
    ("abi_update.hip", "hipcc", ["-Wno-unknown-pragmas"]),
    ("abi_csr.hip", "hipcc", ["-Wno-unknown-pragmas"]),
    ("abi_apply.hip", "hipcc", ["-Wno-unknown-pragmas"]),
    ("abi_gradient.hip", "hipcc", ["-Wno-unknown-pragmas"]),
    ("abi_gradop.hip", "hipcc", ["-Wno-unknown-pragmas"]),
    ("abi_jacobian.hip", "hipcc", ["-Wno-unknown-pragmas"]),
    ("abi_jacobian_reduced.hip", "hipcc", ["-Wno-unknown-pragmas"]),
    ("abi_jacobian_points.hip", "hipcc", ["-Wno-unknown-pragmas"]),
    ("abi_jacobian_dirty.hip", "hipcc", ["-Wno-unknown-pragmas"]),
    # the peer-to-peer exchange of the multi-GPU path (nin_exchange_*): HIP runtime calls only, no kernel
    ("exchange.hip", "hipcc", []),
]


def _run(cmd):
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _hipcc():
    return shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".hpp"))]
    srcs += [os.path.join(os.path.dirname(HERE), "include", "ninpol_amd.h"), os.path.abspath(__file__)]
    return any(os.path.getmtime(s) > t for s in srcs)


def build(force=False, verbose_resources=False):
    if not force and not needs_build():
        return LIB
    os.makedirs(OBJ, exist_ok=True)
    objs = []
    for src, cc, extra in UNITS:
        obj = os.path.join(OBJ, os.path.splitext(src)[0] + ".o")
        common = ["-O3", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, src), "-o", obj]
        if cc == "hipcc":
            cmd = [_hipcc(), f"--offload-arch={ARCH}"] + extra + os.environ.get("NIN_EXTRA_HIPCC_FLAGS", "").split() + common
            if verbose_resources:
                cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
        else:
            cmd = [cc, "-I", os.path.join(ROCM, "include")] + extra + common
        _run(cmd)
        objs.append(obj)
    _run(["g++", "-shared", "-o", LIB] + objs +
         ["-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-lgomp", "-Wl,-rpath," + os.path.join(ROCM, "lib")])
    build_tools()
    return LIB


def build_tools():
    """Stand-alone device test programs (tests/test_gpu_parity.py and tests/test_gpu_face_tau.py run them on the GPU box):
    tools/_bin/test_xstrip, tools/_bin/test_face_tau."""
    tools = os.path.join(os.path.dirname(HERE), "tools")
    os.makedirs(os.path.join(tools, "_bin"), exist_ok=True)
    for name in ("test_xstrip", "test_face_tau"):
        _run([_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-I", CSRC, os.path.join(tools, name + ".hip"), "-o",
              os.path.join(tools, "_bin", name)])


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose_resources="--resources" in sys.argv))
