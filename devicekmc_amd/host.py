"""Host-side mirror of the reference's operator interface for the hot path.

Same names and argument meaning as the reference's C++ host classes, so the parity tests read like
calls into the reference:

  GPUBuffers            gpu_buffers.h:12-162     device-pointer bag (+ sync_HostToGPU / sync_GPUToHost ...)
  Device                Device.h:61-231          setLaplacePotential / updateCharge / updatePotential /
                                                 updatePower / updateTemperature (the USE_CUDA branches of
                                                 potential_solver.cpp, current_solver.cpp, heat_solver.cpp)
  KMCProcess            KMCProcess.h:13-43       executeKMCStep (KMCProcess.cpp:259-373, USE_CUDA branch)

Device memory is owned by torch tensors (plumbing); all computation is done by the HIP library
through the C ABI of include/devicekmc_hip.h.  Nothing here computes on the CPU.
"""
import ctypes as C
import time

import numpy as np
import torch

from . import lib as _lib
from .lib import check, dkmc_gpubuf
from .params import KMCParameters
from .rng import StdMT19937
from .structure import Structure, prepare_device


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class GPUBuffers:
    """gpu_buffers.h:12-162.  Arrays live in torch tensors on ``device``; ``self.c`` is the C struct."""

    F64 = ["site_power", "site_potential_boundary", "site_potential_charge", "site_temperature", "site_CB_edge",
           "atom_power", "atom_CB_edge", "site_x", "site_y", "site_z", "atom_x", "atom_y", "atom_z"]
    I32 = ["site_charge", "atom_charge", "site_element", "atom_element", "site_layer"]

    def __init__(self, layers, site_layer, freq, N, N_atom, site_x, site_y, site_z, nn, sigma, k, lattice, neigh_idx,
                 metals, device="cuda:0"):
        L = _lib.load()
        self.dev = torch.device(device)
        self.N_, self.N_atom_, self.nn_ = int(N), int(N_atom), int(nn)
        self.num_metal_types_ = len(metals)
        self.t = {}
        for n in self.F64:
            self.t[n] = torch.zeros(N, dtype=torch.float64, device=self.dev)
        for n in self.I32:
            self.t[n] = torch.zeros(N, dtype=torch.int32, device=self.dev)
        self.t["atom_virtual_potentials"] = torch.zeros(N_atom + 2, dtype=torch.float64, device=self.dev)
        self.t["neigh_idx"] = torch.as_tensor(np.ascontiguousarray(neigh_idx, dtype=np.int32).reshape(-1)).to(self.dev)
        self.t["site_layer"].copy_(torch.as_tensor(np.ascontiguousarray(site_layer, dtype=np.int32)))
        for n, a in (("site_x", site_x), ("site_y", site_y), ("site_z", site_z)):
            self.t[n].copy_(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)))
        self.t["metal_types"] = torch.as_tensor(np.asarray(metals, dtype=np.int32)).to(self.dev)
        for n, v in (("sigma", [sigma]), ("k", [k]), ("freq", [freq]), ("lattice", list(lattice)), ("T_bg", [0.0])):
            self.t[n] = torch.tensor(v, dtype=torch.float64, device=self.dev)
        self.c = dkmc_gpubuf()
        for n in dkmc_gpubuf._PTRS:
            if n in self.t:
                setattr(self.c, n, self.t[n].data_ptr())
        self.c.N_, self.c.nn_, self.c.N_atom_, self.c.num_metal_types_ = self.N_, self.nn_, self.N_atom_, self.num_metal_types_
        # copytoConstMemory (gpu_buffers.h:102)
        E = [np.array([getattr(l, f) for l in layers], dtype=np.float64) for f in ("E_gen_0", "E_rec_1", "E_diff_2", "E_diff_3")]
        check(L.dkmc_copy_to_const_memory(_np_ptr(E[0]), _np_ptr(E[1]), _np_ptr(E[2]), _np_ptr(E[3]), len(layers)))
        torch.cuda.synchronize(self.dev)

    def __del__(self):
        # the pattern arrays of initialize_sparsity are the only memory of this object that torch does not own
        try:
            if self.__dict__.get("c") is not None and _lib._lib is not None:
                _lib._lib.dkmc_free_sparsity(C.byref(self.c))
        except Exception:
            pass

    def __getattr__(self, name):
        t = self.__dict__.get("t", {})
        if name in t:
            return t[name]
        raise AttributeError(name)

    # gpu_buffers.cpp:10-32
    def sync_HostToGPU(self, device):
        def put(name, arr, dt):
            self.t[name].copy_(torch.as_tensor(np.ascontiguousarray(arr, dtype=dt)))
        put("site_element", device.site_element, np.int32)
        put("site_charge", device.site_charge, np.int32)
        put("site_power", device.site_power, np.float64)
        put("site_CB_edge", device.site_CB_edge, np.float64)
        put("site_potential_boundary", device.site_potential_boundary, np.float64)
        put("site_potential_charge", device.site_potential_charge, np.float64)
        put("site_temperature", device.site_temperature, np.float64)
        self.t["T_bg"].fill_(float(device.T_bg))
        torch.cuda.synchronize(self.dev)

    # gpu_buffers.cpp:34-55
    def sync_GPUToHost(self, device):
        torch.cuda.synchronize(self.dev)
        device.site_element = self.t["site_element"].cpu().numpy()
        device.site_charge = self.t["site_charge"].cpu().numpy()
        device.site_power = self.t["site_power"].cpu().numpy()
        device.site_CB_edge = self.t["site_CB_edge"].cpu().numpy()
        device.site_potential_boundary = self.t["site_potential_boundary"].cpu().numpy()
        device.site_potential_charge = self.t["site_potential_charge"].cpu().numpy()
        device.site_temperature = self.t["site_temperature"].cpu().numpy()
        device.T_bg = float(self.t["T_bg"].item())

    def copy_power_fromGPU(self):
        return self.t["site_power"].cpu().numpy()

    def copy_charge_toGPU(self, charge):
        self.t["site_charge"].copy_(torch.as_tensor(np.ascontiguousarray(charge, dtype=np.int32)))

    def copy_Tbg_toGPU(self, T_bg):
        self.t["T_bg"].fill_(float(T_bg))


def build_neighbor_index_gpu(x, y, z, lattice, pbc, nn_dist, device="cuda:0"):
    """Device.cpp:98-136 + :69-80 on the GPU (cell list, dkmc_build_neighbor_index).  Returns (neigh int32 [N, nn], nn)."""
    L = _lib.load()
    dev = torch.device(device)
    _use_stream(dev)
    tx, ty, tz = (torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in (x, y, z))
    lat = np.ascontiguousarray(lattice, dtype=np.float64)
    nn = C.c_int(0)
    check(L.dkmc_build_neighbor_index(len(x), _ptr(tx), _ptr(ty), _ptr(tz), _np_ptr(lat), int(pbc), nn_dist, C.byref(nn), None))
    out = torch.empty(len(x) * nn.value, dtype=torch.int32, device=dev)
    check(L.dkmc_build_neighbor_index(len(x), _ptr(tx), _ptr(ty), _ptr(tz), _np_ptr(lat), int(pbc), nn_dist, C.byref(nn), _ptr(out)))
    return out.cpu().numpy().reshape(len(x), nn.value), nn.value


def _use_stream(dev):
    check(_lib.load().dkmc_set_stream(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


def _copy_table(call, int_names, double_names, n):
    """One dkmc_copy_* entry point (capacity, the int32 columns, the float64 columns, rows_out) into fresh host columns of n rows: a dict of
    the columns by name, sliced to the rows the call reports."""
    cols = [np.empty(max(n, 0), dtype=np.int32) for _ in int_names] + [np.empty(max(n, 0)) for _ in double_names]
    rows = C.c_int(0)
    check(call(n, *[_np_ptr(c) for c in cols], C.byref(rows)))
    return {k: c[:rows.value] for k, c in zip(tuple(int_names) + tuple(double_names), cols)}


# member sets of the filament analysis (include/devicekmc_hip.h: dkmc_find_clusters); NEUTRAL_ONLY restricts the vacancies to site_charge == 0
METAL, VACANCY, NEUTRAL_ONLY = 1, 2, 4
CLUSTER_INFO = ("n_members", "n_components", "bridged", "bridge_root", "largest_free_size", "rounds")
CLUSTER_TABLE = ("root", "size", "n_vacancy", "flags", "xmin", "xmax")


def find_clusters(index, nn, element, charge, x, metal_types, members, n_left, n_right, capacity=None):
    """dkmc_find_clusters on device tensors (index: N * nn int32; element, charge: N int32; x: N float64; metal_types: int32; charge may be
    None without NEUTRAL_ONLY).  Returns (label: int32 device tensor of N, table: dict of host arrays with min(capacity, n_components) rows --
    capacity None: all of them --, info: dict of CLUSTER_INFO + tip_left_x, tip_right_x, gap_x).  Definitions: include/devicekmc_hip.h."""
    L = _lib.load()
    N = int(element.numel())
    _use_stream(element.device)
    label = torch.empty(N, dtype=torch.int32, device=element.device)
    check(L.dkmc_find_clusters(N, int(nn), _ptr(index), _ptr(element), _ptr(charge) if charge is not None else None, _ptr(x), _ptr(metal_types),
                               int(metal_types.numel()), int(members), int(n_left), int(n_right), _ptr(label)))
    i8, x3 = (C.c_int * 8)(), (C.c_double * 3)()
    check(L.dkmc_get_cluster_info(i8, x3))
    info = dict(zip(CLUSTER_INFO, (int(v) for v in i8)))
    info.update(tip_left_x=x3[0], tip_right_x=x3[1], gap_x=x3[2])
    cap = info["n_components"] if capacity is None else int(capacity)
    return label, _copy_table(L.dkmc_copy_cluster_table, CLUSTER_TABLE[:4], CLUSTER_TABLE[4:], cap), info


GAP_EDGES = ("site_a", "site_b", "root_a", "root_b")
GAP_CHAIN = ("from_site", "to_site")


def find_gaps(label, x, y, z, lattice, pbc, n_left, n_right, r_max):
    """dkmc_find_gaps on device tensors (label: N int32, e.g. the first return value of find_clusters; x, y, z: N float64; lattice: 3 host numbers,
    read with pbc).  Returns (edges: dict of host arrays GAP_EDGES + d2 + dist, one row per edge of the island graph in key order; chain: dict of
    GAP_CHAIN + d2 + dist, the hops from the left contact node to the right one; info: dict of n_components, n_edges, status (0 none, 1 chain,
    2 bridged), n_hops, rounds, pairs_tested, direct = (a, b, dist) or None, bottleneck_d2, bottleneck).  dist = np.sqrt(d2).
    Definitions: include/devicekmc_hip.h."""
    L = _lib.load()
    N = int(label.numel())
    _use_stream(label.device)
    lat = np.ascontiguousarray(lattice, dtype=np.float64)
    check(L.dkmc_find_gaps(N, _ptr(x), _ptr(y), _ptr(z), _np_ptr(lat), int(bool(pbc)), _ptr(label), int(n_left), int(n_right), float(r_max)))
    i8, d2 = (C.c_longlong * 8)(), (C.c_double * 2)()
    check(L.dkmc_get_gap_info(i8, d2))
    edges = _copy_table(L.dkmc_copy_gap_edges, GAP_EDGES, ("d2",), int(i8[1]))
    chain = _copy_table(L.dkmc_copy_gap_chain, GAP_CHAIN, ("d2",), int(i8[3]))
    edges["dist"], chain["dist"] = np.sqrt(edges["d2"]), np.sqrt(chain["d2"])
    info = dict(n_components=int(i8[0]), n_edges=int(i8[1]), status=int(i8[2]), n_hops=int(i8[3]), rounds=int(i8[4]), pairs_tested=int(i8[5]),
                direct=(int(i8[6]), int(i8[7]), float(np.sqrt(d2[1]))) if i8[6] >= 0 else None,
                bottleneck_d2=float(d2[0]), bottleneck=float(np.sqrt(d2[0])))
    return edges, chain, info


PATH_INFO = ("status", "hops", "rounds", "reached_left", "reached_right", "corridor_sites", "constriction_level", "constriction_width")
PATH_PROFILE = ("count", "xmin", "xmax")


def find_paths(index, nn, label, x, n_left, n_right, slack=0):
    """dkmc_find_paths on device tensors (index: N * nn int32; label: N int32, e.g. the first return value of find_clusters; x: N float64 or
    None).  Returns (hops_left, hops_right: int32 device tensors of N; path: host int32 array of the hops + 1 sites of the canonical shortest
    path, empty at status 0; profile: dict of host arrays PATH_PROFILE with hops + slack + 1 rows, empty at status 0; info: dict of PATH_INFO).
    Definitions: include/devicekmc_hip.h."""
    L = _lib.load()
    N = int(label.numel())
    _use_stream(label.device)
    hl = torch.empty(N, dtype=torch.int32, device=label.device)
    hr = torch.empty(N, dtype=torch.int32, device=label.device)
    check(L.dkmc_find_paths(N, int(nn), _ptr(index), _ptr(label), _ptr(x) if x is not None else None, int(n_left), int(n_right), int(slack),
                            _ptr(hl), _ptr(hr)))
    i8 = (C.c_longlong * 8)()
    check(L.dkmc_get_path_info(i8))
    info = dict(zip(PATH_INFO, (int(v) for v in i8)))
    n_path, n_prof = (info["hops"] + 1, info["hops"] + int(slack) + 1) if info["status"] else (0, 0)
    path = _copy_table(L.dkmc_copy_path_sites, ("site",), (), n_path)["site"]
    return hl, hr, path, _copy_table(L.dkmc_copy_path_profile, PATH_PROFILE[:1], PATH_PROFILE[1:], n_prof), info


TRACK_INFO = ("n_prev", "n_now", "n_pairs", "stayed", "joined", "left", "regrouped", "transition", "bridge_prev", "bridge_now",
              "born", "died", "merged", "split", "n_critical")
TRACK_PAIRS = ("prev", "now", "count", "first_site")
TRACK_NOW = ("root", "size", "joined", "n_parents", "main_parent", "flags")
TRACK_PREV = ("root", "size", "left", "n_children", "main_child", "flags")
TRACK_CHANGE = ("none", "stayed", "joined", "left", "regrouped")             # the codes of site_change
TRACK_TRANSITION = ("open", "closed", "ruptured", "bridged")
# flags of the two tables: bits 0, 1 the contacts; bits 2 ... 4 BORN / MERGED / FRAGMENT in the now table, DIED / SPLIT / ABSORBED in the prev table
TRACK_LEFT, TRACK_RIGHT, TRACK_BORN, TRACK_MERGED, TRACK_FRAGMENT = 1, 2, 4, 8, 16
TRACK_DIED, TRACK_SPLIT, TRACK_ABSORBED = 4, 8, 16


def track_clusters(label_prev, label_now, x, n_left, n_right):
    """dkmc_track_clusters on device tensors (label_prev, label_now: N int32, e.g. the first return values of two find_clusters calls -- they may
    be one tensor; x: N float64 or None).  Returns (site_change: int32 device tensor of N, codes TRACK_CHANGE; pairs, now, prev: dicts of host
    int32 arrays TRACK_PAIRS / TRACK_NOW / TRACK_PREV; critical: host int32 array of the sites that closed or broke the filament; info: dict of
    TRACK_INFO + critical_xmin, critical_xmax).  Definitions: include/devicekmc_hip.h."""
    L = _lib.load()
    N = int(label_now.numel())
    if int(label_prev.numel()) != N:
        raise ValueError("track_clusters: label_prev has %d sites, label_now %d" % (int(label_prev.numel()), N))
    _use_stream(label_now.device)
    change = torch.empty(N, dtype=torch.int32, device=label_now.device)
    check(L.dkmc_track_clusters(N, _ptr(label_prev), _ptr(label_now), _ptr(x) if x is not None else None, int(n_left), int(n_right), _ptr(change)))
    i16, x2 = (C.c_longlong * 16)(), (C.c_double * 2)()
    check(L.dkmc_get_track_info(i16, x2))
    info = dict(zip(TRACK_INFO, (int(v) for v in i16)))
    info.update(critical_xmin=x2[0], critical_xmax=x2[1])
    pairs = _copy_table(L.dkmc_copy_track_pairs, TRACK_PAIRS, (), info["n_pairs"])
    now = _copy_table(L.dkmc_copy_track_now, TRACK_NOW, (), info["n_now"])
    prev = _copy_table(L.dkmc_copy_track_prev, TRACK_PREV, (), info["n_prev"])
    critical = _copy_table(L.dkmc_copy_track_critical, ("site",), (), info["n_critical"])["site"]
    return change, pairs, now, prev, critical, info


CUT_INFO = ("status", "path_len", "cut_sites", "necks", "longest_neck", "longest_neck_first", "bypasses", "offpath_components", "offpath_members",
            "max_bypass", "chord_positions", "rounds")
CUT_PATH = ("site", "n_bypass", "chord", "cut")
CUT_BYPASSES = ("root", "size", "lo", "hi")
CUT_NECKS = ("first", "last", "xmin", "xmax")
CUT_ROLE = ("none", "cut", "path", "bypass", "side", "apart")                # the codes of site_role


def find_cuts(index, nn, label, x, n_left, n_right, path):
    """dkmc_find_cuts on device tensors (index: N * nn int32; label: N int32, e.g. the first return value of find_clusters; x: N float64 or
    None; path: the sites of a left-to-right path, normally the third return value of find_paths -- a host array or an int32 device tensor;
    empty or None: the status 0 answer).  Returns (site_role: int32 device tensor of N, codes CUT_ROLE; site_bypass: int32 device tensor of N;
    path_table, bypasses, necks: dicts of host arrays CUT_PATH / CUT_BYPASSES / CUT_NECKS; info: dict of CUT_INFO).
    Definitions: include/devicekmc_hip.h."""
    L = _lib.load()
    N = int(label.numel())
    _use_stream(label.device)
    if path is None:
        path = np.zeros(0, dtype=np.int32)
    if not torch.is_tensor(path):
        path = torch.as_tensor(np.ascontiguousarray(path, dtype=np.int32).reshape(-1))
    path = path.to(device=label.device, dtype=torch.int32).contiguous()
    n_path = int(path.numel())
    role = torch.empty(N, dtype=torch.int32, device=label.device)
    bypass = torch.empty(N, dtype=torch.int32, device=label.device)
    check(L.dkmc_find_cuts(N, int(nn), _ptr(index), _ptr(label), _ptr(x) if x is not None else None, int(n_left), int(n_right),
                           _ptr(path) if n_path else None, n_path, _ptr(role), _ptr(bypass)))
    i16 = (C.c_longlong * 16)()
    check(L.dkmc_get_cut_info(i16))
    info = dict(zip(CUT_INFO, (int(v) for v in i16)))
    path_table = _copy_table(L.dkmc_copy_cut_path, CUT_PATH, (), info["path_len"])
    bypasses = _copy_table(L.dkmc_copy_cut_bypasses, CUT_BYPASSES, (), info["bypasses"])
    necks = _copy_table(L.dkmc_copy_cut_necks, CUT_NECKS[:2], CUT_NECKS[2:], info["necks"])
    return role, bypass, path_table, bypasses, necks, info


FLOW_INFO = ("status", "width", "left_shore", "right_shore", "shared_cut", "interior", "near_left", "near_right", "searches", "rounds",
             "longest_strand", "shortest_strand")
FLOW_STRANDS = ("first_site", "last_site", "length", "offset", "left_seed", "right_seed", "cut_left_site", "cut_left_pos", "cut_right_site",
                "cut_right_pos")
FLOW_ZONE = ("member", "left_shore", "left_cut", "right_cut", "right_shore")   # bit k of site_zone


def find_flow(index, nn, label, x, n_left, n_right, max_strands=64):
    """dkmc_find_flow on device tensors (index: N * nn int32; label: N int32, e.g. the first return value of find_clusters; x: N float64 or
    None; max_strands: 1 ... 4096, the search stops with status 3 once that many disjoint strands exist).  Returns (site_zone: int32 device
    tensor of N, bit k = FLOW_ZONE[k]; site_strand: int32 device tensor of N; strands: dict of host int32 arrays FLOW_STRANDS, one row per strand;
    strand_sites: host int32 array, the strands' sites in table order; info: dict of FLOW_INFO + cut_left_xmin, cut_left_xmax, cut_right_xmin,
    cut_right_xmax).  Definitions: include/devicekmc_hip.h."""
    L = _lib.load()
    N = int(label.numel())
    _use_stream(label.device)
    zone = torch.empty(N, dtype=torch.int32, device=label.device)
    strand = torch.empty(N, dtype=torch.int32, device=label.device)
    check(L.dkmc_find_flow(N, int(nn), _ptr(index), _ptr(label), _ptr(x) if x is not None else None, int(n_left), int(n_right), int(max_strands),
                           _ptr(zone), _ptr(strand)))
    i16, x4 = (C.c_longlong * 16)(), (C.c_double * 4)()
    check(L.dkmc_get_flow_info(i16, x4))
    info = dict(zip(FLOW_INFO, (int(v) for v in i16)))
    info.update(cut_left_xmin=x4[0], cut_left_xmax=x4[1], cut_right_xmin=x4[2], cut_right_xmax=x4[3])
    strands = _copy_table(L.dkmc_copy_flow_strands, FLOW_STRANDS, (), max(info["width"], 0))
    sites = _copy_table(L.dkmc_copy_flow_strand_sites, ("site",), (), int(strands["length"].sum()))["site"]
    return zone, strand, strands, sites, info


# rate census of an event table (include/devicekmc_hip.h: dkmc_event_rate_census); classes in the order of the EVENTTYPE enum
EVENT_CLASSES = ("gen", "rec", "vdiff", "idiff")


def _census_dict(info):
    """The 16 doubles of the census as named entries + the per-class rate-weighted mean temperature (NaN for a class without rate)."""
    v = [float(x) for x in info]
    d = {"n_slots": {c: int(v[k]) for k, c in enumerate(EVENT_CLASSES)},
         "rate": {c: v[4 + k] for k, c in enumerate(EVENT_CLASSES)},
         "rate_temperature": {c: v[8 + k] for k, c in enumerate(EVENT_CLASSES)},
         "max_rate": v[12], "max_rate_slot": int(v[13]), "n_nonfinite": int(v[14]), "n_live": int(v[15]), "info16": v}
    d["rate_total"] = v[4] + v[5] + v[6] + v[7]
    d["mean_temperature"] = {c: (v[8 + k] / v[4 + k] if v[4 + k] > 0 else float("nan")) for k, c in enumerate(EVENT_CLASSES)}
    return d


def event_rate_census(neigh_idx, nn, element, ev_prob, temperature=None):
    """dkmc_event_rate_census on device tensors (neigh_idx: N * nn int32; element: N int32; ev_prob: N * nn float64, e.g. the table of
    dkmc_build_event_list_T; temperature: N float64 or None).  Returns the dict of _census_dict.  Definitions: include/devicekmc_hip.h."""
    L = _lib.load()
    _use_stream(element.device)
    info = (C.c_double * 16)()
    check(L.dkmc_event_rate_census(int(element.numel()), int(nn), _ptr(neigh_idx), _ptr(element),
                                   _ptr(temperature) if temperature is not None else None, _ptr(ev_prob), info))
    return _census_dict(info)


class Device:
    """Device.h:61-231 (USE_CUDA build): host copy of the site fields + the thin callers of the GPU path."""

    def __init__(self, structure: Structure, p: KMCParameters, gpu_neighbors=None):
        """gpu_neighbors: device string (e.g. "cuda:0") to build the neighbour index with the HIP cell list instead of
        the host k-d tree (same result; minutes faster at 1e6 sites)."""
        self.p = p
        self.N = structure.N
        self.site_x, self.site_y, self.site_z = structure.x, structure.y, structure.z
        neigh = None
        if gpu_neighbors:
            neigh = build_neighbor_index_gpu(structure.x, structure.y, structure.z, p.lattice, p.pbc, p.nn_dist, gpu_neighbors)
        self.site_element, self.neigh_idx, self.max_num_neighbors, self.site_layer = prepare_device(structure, p, neigh)
        self.lattice, self.pbc, self.nn_dist, self.sigma, self.k = p.lattice, p.pbc, p.nn_dist, p.sigma, p.k
        self.T_bg = p.background_temp
        self.site_charge = np.zeros(self.N, dtype=np.int32)
        self.site_CB_edge = np.zeros(self.N)
        self.site_potential_boundary = np.zeros(self.N)
        self.site_potential_charge = np.zeros(self.N)
        self.site_power = np.zeros(self.N)
        self.site_temperature = np.full(self.N, self.T_bg)
        self.N_atom = int(((self.site_element != 0) & (self.site_element != 1)).sum())
        self.imacro = 0.0

    def make_gpubuf(self, device="cuda:0") -> GPUBuffers:
        """kmc_main.cpp:116-121: GPUBuffers ctor + sync_HostToGPU + initialize_sparsity."""
        p = self.p
        g = GPUBuffers(p.layers, self.site_layer, p.freq, self.N, self.N_atom, self.site_x, self.site_y, self.site_z,
                       self.max_num_neighbors, self.sigma, self.k, self.lattice, self.neigh_idx, list(p.metals), device)
        g.sync_HostToGPU(self)
        _use_stream(g.dev)
        _lib.load().dkmc_set_cg_tolerance(p.cg_tol)
        check(_lib.load().dkmc_initialize_sparsity(C.byref(g.c), int(p.pbc), p.nn_dist, p.num_atoms_first_layer))
        return g

    # potential_solver.cpp:4-19
    def setLaplacePotential(self, gpubuf: GPUBuffers, p: KMCParameters, Vd: float):
        n = p.num_atoms_first_layer
        gpubuf.sync_HostToGPU(self)
        _use_stream(gpubuf.dev)
        _lib.load().dkmc_set_cg_tolerance(p.cg_tol)            # the parameters are authoritative for every solve (the engine's tolerance is process-wide)
        _lib.load().dkmc_set_cb_edge_domain(1 if p.cb_edge_domain == "atoms" else 0)
        check(_lib.load().dkmc_update_CB_edge_gpu_sparse(C.byref(gpubuf.c), self.N, n, n, Vd, int(self.pbc), p.high_G, p.low_G,
                                                         self.nn_dist, len(p.metals)))
        gpubuf.sync_GPUToHost(self)

    # potential_solver.cpp:142-160
    def updateCharge(self, gpubuf: GPUBuffers, metals=None):
        t0 = time.perf_counter()
        _use_stream(gpubuf.dev)
        check(_lib.load().dkmc_update_charge_gpu(_ptr(gpubuf.site_element), _ptr(gpubuf.site_charge), _ptr(gpubuf.neigh_idx),
                                                 gpubuf.N_, gpubuf.nn_, _ptr(gpubuf.metal_types), gpubuf.num_metal_types_))
        return {"Z - calculation time - charge [s]": time.perf_counter() - t0}

    # potential_solver.cpp:232-285
    def updatePotential(self, gpubuf: GPUBuffers, p: KMCParameters, Vd: float, kmc_step_count: int = 0, sync=False):
        L = _lib.load()
        n = p.num_atoms_first_layer
        _use_stream(gpubuf.dev)
        L.dkmc_set_cg_tolerance(p.cg_tol)
        t0 = time.perf_counter()
        check(L.dkmc_background_potential_gpu_sparse(C.byref(gpubuf.c), self.N, n, n, Vd, int(self.pbc), p.high_G, p.low_G,
                                                     self.nn_dist, len(p.metals), kmc_step_count))
        if sync:
            torch.cuda.synchronize(gpubuf.dev)
        t1 = time.perf_counter()
        check(L.dkmc_poisson_gridless_gpu(p.num_atoms_contact, int(self.pbc), gpubuf.N_, _ptr(gpubuf.lattice), _ptr(gpubuf.sigma),
                                          _ptr(gpubuf.k), _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z),
                                          _ptr(gpubuf.site_charge), _ptr(gpubuf.site_potential_charge)))
        if sync:
            torch.cuda.synchronize(gpubuf.dev)
        t2 = time.perf_counter()
        return {"Z - calculation time - potential from boundaries [s]": t1 - t0,
                "Z - calculation time - potential from charges [s]": t2 - t1}

    # current_solver.cpp:4-47 (constants :8-17)
    def updatePower(self, gpubuf: GPUBuffers, p: KMCParameters, Vd: float):
        t0 = time.perf_counter()
        _use_stream(gpubuf.dev)
        imacro = C.c_double(0.0)
        n = p.num_atoms_first_layer
        _lib.load().dkmc_set_cg_tolerance(p.cg_tol)
        check(_lib.load().dkmc_update_power_gpu_sparse(C.byref(gpubuf.c), n, n, p.num_layers_contact, Vd, int(self.pbc),
                                                       p.X_high_G, p.X_low_G, p.X_loop_G, p.G0, p.X_tol, self.nn_dist, p.m_e, p.V0,
                                                       len(p.metals), C.byref(imacro), int(p.solve_heating_local),
                                                       int(p.solve_heating_global), 1.0))
        self.imacro = imacro.value
        if _lib.load().dkmc_get_current_map():
            self._fetch_current_map(gpubuf)
        return {"Current [uA]": self.imacro * 1e6, "Z - calculation time - dissipated power [s]": time.perf_counter() - t0}

    CURRENT_MAP_INFO = ("I_macro", "I_driver0", "max_node_defect", "sum_current", "sum_current_tunnel", "rows", "tile_passes", "reserved")

    def _fetch_current_map(self, gpubuf: GPUBuffers):
        """dkmc_set_current_map(1): the atom-resolved current map of the solve just done (definitions: include/devicekmc_hip.h).
        site_current = thr_all, site_current_tunnel = thr_tun, site_tunnel_outflow = net_tun, per site, in amperes."""
        L = _lib.load()
        a, t, o, info = np.empty(self.N), np.empty(self.N), np.empty(self.N), (C.c_double * 8)()
        check(L.dkmc_copy_current_map_from_gpu(C.byref(gpubuf.c), _np_ptr(a), _np_ptr(t), _np_ptr(o)))
        check(L.dkmc_get_current_map_info(C.byref(gpubuf.c), info))
        self.site_current, self.site_current_tunnel, self.site_tunnel_outflow = a, t, o
        self.current_map_info = dict(zip(self.CURRENT_MAP_INFO, list(info)))

    def tunnel_current_profile(self, cuts):
        """Tunnelling current crossing the plane x = cut, for every cut: the sum of site_tunnel_outflow over the sites with site_x <= cut
        (the tunnelling block is symmetric, so the pairs inside that set cancel).  Divide by imacro for the tunnelling share."""
        x, out = np.asarray(self.site_x), np.asarray(self.site_tunnel_outflow)
        return np.array([out[x <= c].sum() for c in np.atleast_1d(np.asarray(cuts, dtype=np.float64))])

    def find_clusters(self, gpubuf: GPUBuffers, members=METAL | VACANCY, link_index=None, n_left=None, n_right=None, capacity=None):
        """Filament analysis on the device (dkmc_find_clusters; definitions: include/devicekmc_hip.h): the connected components of the member
        sites of gpubuf's CURRENT site_element (and site_charge, with NEUTRAL_ONLY) over gpubuf.neigh_idx, or over link_index = (int32 device
        tensor of N * nn, nn) -- e.g. build_neighbor_index_gpu at a larger radius, moved to the device -- for a gap-tolerant filament.  n_left /
        n_right: sites of the contact seeds, by default get_num_in_contacts(num_atoms_first_layer) on either side.  Changes nothing in gpubuf.
        Returns (labels: host int32 array, table, info) and keeps them as site_cluster, cluster_table, cluster_info."""
        n_left, n_right = self.contact_seeds(n_left, n_right)
        index, nn = self._links(gpubuf, link_index)
        label, table, info = find_clusters(index, nn, gpubuf.site_element, gpubuf.site_charge, gpubuf.site_x, gpubuf.metal_types, members,
                                           n_left, n_right, capacity)
        self._cluster_label_prev = getattr(self, "_cluster_label", None)       # the tensor this call replaces (a reference), for track_clusters
        self._cluster_label = label                # the device tensor, for find_gaps
        self.site_cluster, self.cluster_table, self.cluster_info = label.cpu().numpy(), table, info
        return self.site_cluster, table, info

    def track_clusters(self, gpubuf: GPUBuffers, label_prev=None, label_now=None, n_left=None, n_right=None):
        """Cluster tracking on the device (dkmc_track_clusters; definitions: include/devicekmc_hip.h) between the labels of the last two
        find_clusters calls -- the earlier one as prev -- or between label_prev / label_now (int32 device tensors of N; one given alone replaces
        that side): per-site change codes, the distinct (prev, now) pairs, one lineage row per component of either side, the transition of the
        bridging verdict and the sites that closed or broke the filament, with the contact seeds of find_clusters.  Changes nothing in gpubuf.
        Returns (site_change: host int32 array, pairs, now, prev, critical, info) and keeps them as site_change, track_pairs, track_now,
        track_prev, track_critical, track_info."""
        if label_now is None:
            label_now = getattr(self, "_cluster_label", None)
        if label_prev is None:
            label_prev = getattr(self, "_cluster_label_prev", None)
        if label_prev is None or label_now is None:
            raise ValueError("track_clusters compares two labellings: fewer than two find_clusters calls were made on this Device "
                             "(or pass label_prev and label_now)")
        n_left, n_right = self.contact_seeds(n_left, n_right)
        change, pairs, now, prev, critical, info = track_clusters(label_prev, label_now, gpubuf.site_x, n_left, n_right)
        self.site_change = change.cpu().numpy()
        self.track_pairs, self.track_now, self.track_prev, self.track_critical, self.track_info = pairs, now, prev, critical, info
        return self.site_change, pairs, now, prev, critical, info

    def _labels_or(self, label, otherwise):
        """The labels an analysis runs on: label if given, else the device tensor of the last find_clusters.  Where there is neither, otherwise
        decides: an exception is raised, a callable is called and has to make that find_clusters call."""
        if label is not None:
            return label
        if getattr(self, "_cluster_label", None) is None:
            if isinstance(otherwise, Exception):
                raise otherwise
            otherwise()
        return self._cluster_label

    def _labels_and_seeds(self, label, otherwise, n_left, n_right):
        """(label, n_left, n_right) of an analysis: the labels by _labels_or -- first, with n_left / n_right as given --, then contact_seeds."""
        label = self._labels_or(label, otherwise)
        return (label,) + self.contact_seeds(n_left, n_right)

    @staticmethod
    def _links(gpubuf, link_index):
        """(index, nn) an analysis walks: link_index = (int32 device tensor of N * nn, nn) if given, else gpubuf's neighbour index."""
        return (gpubuf.neigh_idx, gpubuf.nn_) if link_index is None else link_index

    def find_gaps(self, gpubuf: GPUBuffers, r_max=10.0, label=None, n_left=None, n_right=None):
        """Gap analysis on the device (dkmc_find_gaps; definitions: include/devicekmc_hip.h) over the labels of the last find_clusters -- one with
        the default members is run if there is none -- or over label (int32 device tensor of N): the island graph within r_max, the tunnelling
        chain between the contact clusters with its bottleneck hop, and the direct tip-to-tip gap, with this device's pbc and lattice and the
        contact seeds of find_clusters.  Changes nothing in gpubuf.  Returns (edges, chain, info) and keeps them as gap_edges, gap_chain, gap_info."""
        label, n_left, n_right = self._labels_and_seeds(label, lambda: self.find_clusters(gpubuf, n_left=n_left, n_right=n_right), n_left, n_right)
        self.gap_edges, self.gap_chain, self.gap_info = find_gaps(label, gpubuf.site_x, gpubuf.site_y, gpubuf.site_z, self.lattice, self.pbc,
                                                                  n_left, n_right, r_max)
        return self.gap_edges, self.gap_chain, self.gap_info

    def find_paths(self, gpubuf: GPUBuffers, slack=0, label=None, link_index=None, n_left=None, n_right=None):
        """Conduction-path analysis on the device (dkmc_find_paths; definitions: include/devicekmc_hip.h) over the labels of the last
        find_clusters -- one with the default members is run if there is none -- or over label (int32 device tensor of N): the hop distance of
        every member from either contact over gpubuf.neigh_idx, or over link_index = (int32 device tensor of N * nn, nn), the canonical shortest
        path, the level profile of the corridor of the walks at most slack links longer and its constriction, with the contact seeds of
        find_clusters.  Changes nothing in gpubuf.  Returns (hops_left, hops_right: host int32 arrays, path, profile, info) and keeps them as
        site_hops_left, site_hops_right, path_sites, path_profile, path_info."""
        label, n_left, n_right = self._labels_and_seeds(label, lambda: self.find_clusters(gpubuf, n_left=n_left, n_right=n_right), n_left, n_right)
        index, nn = self._links(gpubuf, link_index)
        hl, hr, path, profile, info = find_paths(index, nn, label, gpubuf.site_x, n_left, n_right, slack)
        self.site_hops_left, self.site_hops_right = hl.cpu().numpy(), hr.cpu().numpy()
        self.path_sites, self.path_profile, self.path_info = path, profile, info
        return self.site_hops_left, self.site_hops_right, path, profile, info

    def find_cuts(self, gpubuf: GPUBuffers, path=None, label=None, link_index=None, n_left=None, n_right=None):
        """Cut-site analysis on the device (dkmc_find_cuts; definitions: include/devicekmc_hip.h) over the labels of the last find_clusters -- or
        over label (int32 device tensor of N) -- and, by default, the path of the last find_paths (path_sites; an empty one gives status 0): the
        sites every conducting path between the contacts crosses, the off-path components that bypass the others, and the necks, over
        gpubuf.neigh_idx or link_index = (int32 device tensor of N * nn, nn) -- the index the path was found on -- with the contact seeds of
        find_clusters.  Changes nothing in gpubuf.  Returns (site_role, site_bypass: host int32 arrays, path_table, bypasses, necks, info) and
        keeps them as site_role, site_bypass, cut_path, cut_bypasses, cut_necks, cut_info."""
        label, n_left, n_right = self._labels_and_seeds(
            label, ValueError("find_cuts runs on the labels of a find_clusters call: none was made on this Device (or pass label)"), n_left, n_right)
        if path is None:
            path = getattr(self, "path_sites", None)
            if path is None:
                raise ValueError("find_cuts takes a left-to-right path: no find_paths call was made on this Device (or pass path)")
        index, nn = self._links(gpubuf, link_index)
        role, bypass, table, bypasses, necks, info = find_cuts(index, nn, label, gpubuf.site_x, n_left, n_right, path)
        self.site_role, self.site_bypass = role.cpu().numpy(), bypass.cpu().numpy()
        self.cut_path, self.cut_bypasses, self.cut_necks, self.cut_info = table, bypasses, necks, info
        return self.site_role, self.site_bypass, table, bypasses, necks, info

    def find_flow(self, gpubuf: GPUBuffers, max_strands=64, label=None, link_index=None, n_left=None, n_right=None):
        """Min-cut analysis on the device (dkmc_find_flow; definitions: include/devicekmc_hip.h) over the labels of the last find_clusters -- one
        with the default members is run if there is none -- or over label (int32 device tensor of N): W, the largest number of conducting paths
        between the contacts that share no atom, the minimum separators nearest either contact with their shores, and one canonical family of W
        strands, over gpubuf.neigh_idx or link_index = (int32 device tensor of N * nn, nn), with the contact seeds of find_clusters.  Changes
        nothing in gpubuf.  Returns (site_zone, site_strand: host int32 arrays, strands, strand_sites, info) and keeps them as site_zone,
        site_strand, flow_strands, flow_strand_sites, flow_info."""
        label, n_left, n_right = self._labels_and_seeds(label, lambda: self.find_clusters(gpubuf, n_left=n_left, n_right=n_right), n_left, n_right)
        index, nn = self._links(gpubuf, link_index)
        zone, strand, strands, sites, info = find_flow(index, nn, label, gpubuf.site_x, n_left, n_right, max_strands)
        self.site_zone, self.site_strand = zone.cpu().numpy(), strand.cpu().numpy()
        self.flow_strands, self.flow_strand_sites, self.flow_info = strands, sites, info
        return self.site_zone, self.site_strand, strands, sites, info

    # heat_solver.cpp:250-312 (global branch; computed on the device instead of copy_power_fromGPU + host sum)
    def updateTemperature(self, gpubuf: GPUBuffers, p: KMCParameters, step_time: float):
        result = {}
        if p.solve_heating_global:
            _use_stream(gpubuf.dev)
            P = C.c_double(0.0)
            check(_lib.load().dkmc_update_temperature_global_analytic(_ptr(gpubuf.site_power), _ptr(gpubuf.T_bg), gpubuf.N_, step_time,
                                                                      p.dissipation_constant, p.t_ox, p.A, p.c_p, C.byref(P)))
            self.T_bg = float(gpubuf.T_bg.item())
            result["Global temperature [K]"] = self.T_bg
            result["Total dissipated power [mW]"] = P.value * 1e3
        elif p.solve_heating_local:
            # heat_solver.cpp:286-308; the dense host inverses of the reference are replaced by sparse solves on the device
            _use_stream(gpubuf.dev)
            ns, steady, iters, T = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
            check(_lib.load().dkmc_update_temperature_local(C.byref(gpubuf.c), step_time, p.delta_t, p.tau, p.background_temp,
                                                            p.k_th_interface, p.k_th_vacancies, self.nn_dist, p.num_atoms_contact,
                                                            C.byref(ns), C.byref(steady), C.byref(iters), C.byref(T)))
            self.T_bg = T.value
            self.last_heat_solves, self.last_heat_steady, self.last_heat_cg_iters = ns.value, bool(steady.value), iters.value
            self.last_heat_info = None
            if hasattr(_lib.load(), "dkmc_get_heat_info"):
                info = (C.c_longlong * 8)()
                check(_lib.load().dkmc_get_heat_info(info))
                self.last_heat_info = dict(zip(("form", "rows", "stored_words", "sub_steps", "host_syncs", "resumed_sub_steps", "bytes_per_iteration"),
                                               list(info)[:7]))
            result["Global temperature [K]"] = self.T_bg
        return result

    # heat_solver.cpp:5-37
    def get_num_in_contacts(self, num_atoms_contact: int, contact_name: str) -> int:
        el, N = self.site_element, self.N
        nondef = np.flatnonzero(el != 0)                      # positions of the non-DEFECT sites
        if contact_name == "left":
            return 0 if num_atoms_contact <= 0 else int(nondef[num_atoms_contact - 1]) + 1
        return 0 if num_atoms_contact <= 0 else N - int(nondef[len(nondef) - num_atoms_contact])

    def contact_seeds(self, n_left=None, n_right=None):
        """(n_left, n_right) of the contact seeds of find_clusters / find_gaps: a given value as it is, otherwise
        get_num_in_contacts(num_atoms_first_layer) on that side."""
        k = self.p.num_atoms_first_layer
        return (self.get_num_in_contacts(k, "left") if n_left is None else n_left,
                self.get_num_in_contacts(k, "right") if n_right is None else n_right)

    # heat_solver.cpp:40-246 (kmc_main.cpp:90-94: once, when solve_heating_local is set)
    def constructLaplacian(self, gpubuf: GPUBuffers, p: KMCParameters):
        _use_stream(gpubuf.dev)
        N_metals = int(np.isin(self.site_element, list(p.metals)).sum())                      # Device.cpp:45-50
        self.N_left_tot = self.get_num_in_contacts(p.num_atoms_contact, "left")
        self.N_right_tot = self.get_num_in_contacts(N_metals - p.num_atoms_contact, "right")
        self.N_interface = self.N - self.N_left_tot - self.N_right_tot
        gamma = 1.0 / (p.delta * ((p.k_th_interface / p.k_th_metal) + 1.0))
        check(_lib.load().dkmc_construct_laplacian(C.byref(gpubuf.c), self.N_left_tot, self.N_right_tot, gamma))


class KMCProcess:
    """KMCProcess.h:13-43: owns the KMC random stream and the per-site layer ids."""

    def __init__(self, device: Device, freq: float):
        self.freq = freq
        self.random_generator = StdMT19937(device.p.rnd_seed_kmc)
        self.layers = device.p.layers
        self.site_layer = device.site_layer
        self.batch = 64            # events worth of random numbers handed to the device per launch
        self.last_event_log = None
        self.last_event_census = None     # device.p.event_census: the rate census of the last step's table (host._census_dict)

    # KMCProcess.cpp:259-373 (USE_CUDA branch) -> execute_kmc_step_gpu (kmc_events.cu:146-365)
    def executeKMCStep(self, gpubuf: GPUBuffers, device: Device, want_log=False):
        L = _lib.load()
        t0 = time.perf_counter()
        _use_stream(gpubuf.dev)
        g = gpubuf
        # the parameters are authoritative for the rate model on every call (the engine's switches are process-wide)
        L.dkmc_set_event_temperature(int(device.p.event_temperature))
        L.dkmc_set_event_census(1 if device.p.event_census else 0)
        total_events, logs, resume = 0, [], 0
        self.last_n_events = 0
        self.last_event_census = None
        while True:
            probe = self.random_generator.copy()
            u = np.ascontiguousarray(probe.uniform_batch(2 * self.batch))
            n_ev, exhausted, et = C.c_int(0), C.c_int(0), C.c_double(0.0)
            log = np.zeros((self.batch, 4), dtype=np.int32) if want_log else None
            check(L.dkmc_execute_kmc_step_gpu(device.N, device.max_num_neighbors, _ptr(g.neigh_idx), _ptr(g.site_layer), _ptr(g.lattice),
                                              int(device.pbc), _ptr(g.T_bg), _ptr(g.freq), _ptr(g.sigma), _ptr(g.k),
                                              _ptr(g.site_x), _ptr(g.site_y), _ptr(g.site_z), _ptr(g.site_potential_boundary),
                                              _ptr(g.site_potential_charge), _ptr(g.site_temperature), _ptr(g.site_element),
                                              _ptr(g.site_charge), _np_ptr(u), len(u), resume,
                                              C.byref(n_ev), C.byref(exhausted), _np_ptr(log) if want_log else None, C.byref(et)))
            self.random_generator.skip(2 * n_ev.value)       # exactly the numbers the reference would have drawn
            total_events += n_ev.value
            if want_log:
                logs.append(log[:n_ev.value])
            if not exhausted.value:
                break
            resume = 1
        if want_log:
            self.last_event_log = np.concatenate(logs) if logs else np.zeros((0, 4), dtype=np.int32)
        self.last_n_events = total_events
        if L.dkmc_get_event_census_on():
            info = (C.c_double * 16)()
            check(L.dkmc_get_event_census(info))
            self.last_event_census = _census_dict(info)
        return {"Z - calculation time - kmc events [s]": time.perf_counter() - t0}, et.value


def save_restart(path, device: Device, sim: KMCProcess, gpubuf: GPUBuffers, kmc_time=0.0, kmc_step_count=0):
    """Device::writeSnapshot (Device.cpp:236-252) + the state it drops (io.write_restart): after load_restart the run continues with
    the same event sequence, bit for bit.  The start vector of the next current solve is part of that state in both modes of
    dkmc_set_current_warm_start: gpubuf.atom_virtual_potentials (mode 0 reads it) and the library's private unscaled copy of the last
    solution (mode 1, the default; dkmc_get_current_warm_vector) together with the solutions of the block-CG's auxiliary columns
    (dkmc_get_current_warm_aux)."""
    from . import io
    L = _lib.load()
    gpubuf.sync_GPUToHost(device)
    n = C.c_int(0)
    check(L.dkmc_get_current_warm_vector(C.byref(gpubuf.c), None, 0, C.byref(n)))
    warm = np.zeros(n.value)
    if n.value:
        check(L.dkmc_get_current_warm_vector(C.byref(gpubuf.c), _np_ptr(warm), n.value, C.byref(n)))
    na = C.c_longlong(0)
    check(L.dkmc_get_current_warm_aux(C.byref(gpubuf.c), None, 0, C.byref(na)))
    warm_aux = np.zeros(na.value)
    if na.value:
        check(L.dkmc_get_current_warm_aux(C.byref(gpubuf.c), _np_ptr(warm_aux), na.value, C.byref(na)))
    state = dict(site_charge=device.site_charge, site_potential_boundary=device.site_potential_boundary,
                 site_potential_charge=device.site_potential_charge, site_power=device.site_power,
                 site_temperature=device.site_temperature, site_CB_edge=device.site_CB_edge,
                 atom_virtual_potentials=gpubuf.atom_virtual_potentials.cpu().numpy(), current_warm_vector=warm, current_warm_aux=warm_aux,
                 T_bg=float(device.T_bg), kmc_time=float(kmc_time), kmc_step_count=int(kmc_step_count),
                 rnd_seed_kmc=int(sim.random_generator.seed), kmc_rng_raw_draws=int(sim.random_generator.n_raw),
                 current_warm_start=int(L.dkmc_get_current_warm_start()), N_atom_buffer=int(gpubuf.N_atom_))
    io.write_restart(path, device.site_element, device.site_x, device.site_y, device.site_z, state)


def load_restart(path, p: KMCParameters, device="cuda:0", gpu_neighbors=None):
    """kmc_main.cpp:65-80 (restart = 1: the snapshot is the site list, no substoichiometry pass) + the sidecar state.
    Returns (Device, KMCProcess, GPUBuffers, state)."""
    import copy as _copy
    from . import io
    s, state = io.read_restart(path)
    p = _copy.copy(p); p.pristine = False
    dev = Device(s, p, gpu_neighbors=gpu_neighbors)
    sim = KMCProcess(dev, p.freq)
    gb = dev.make_gpubuf(device)
    if state is not None:
        dev.site_charge = np.asarray(state["site_charge"], dtype=np.int32)
        dev.site_potential_boundary = np.asarray(state["site_potential_boundary"], dtype=np.float64)
        dev.site_potential_charge = np.asarray(state["site_potential_charge"], dtype=np.float64)
        dev.site_power = np.asarray(state["site_power"], dtype=np.float64)
        dev.site_temperature = np.asarray(state["site_temperature"], dtype=np.float64)
        dev.site_CB_edge = np.asarray(state["site_CB_edge"], dtype=np.float64)
        dev.T_bg = float(state["T_bg"])
        gb.sync_HostToGPU(dev)
        warm = np.asarray(state["current_warm_vector"], dtype=np.float64) if "current_warm_vector" in state else np.zeros(0)
        if int(state.get("current_warm_start", 0)) != 0 and "current_warm_vector" not in state:
            raise ValueError("restart sidecar was written in warm-start mode 1 by a version that did not save the private start vector: "
                             "a bit-identical continuation is not possible")
        check(_lib.load().dkmc_set_current_warm_vector(C.byref(gb.c), _np_ptr(warm) if len(warm) else None, len(warm)))
        waux = np.asarray(state["current_warm_aux"], dtype=np.float64) if "current_warm_aux" in state else np.zeros(0)
        check(_lib.load().dkmc_set_current_warm_aux(C.byref(gb.c), _np_ptr(waux) if len(waux) else None, len(waux)))
        # the start vector of the next current solve: entries [0, Na + 1) of the saved buffer are read (Na = atoms of the snapshot).  The
        # buffer of the saved run was sized for ITS initial atom count, this one for the snapshot's: the used part must fit both.
        m = np.asarray(state["atom_virtual_potentials"], dtype=np.float64)
        need = dev.N_atom + 1
        if len(m) < need or gb.atom_virtual_potentials.numel() < need:
            raise ValueError("restart sidecar holds %d virtual potentials, the snapshot needs %d" % (len(m), need))
        n = min(len(m), gb.atom_virtual_potentials.numel())
        gb.atom_virtual_potentials.zero_()
        gb.atom_virtual_potentials[:n].copy_(torch.as_tensor(m[:n]))
        sim.random_generator = StdMT19937.at_position(int(state["rnd_seed_kmc"]), int(state["kmc_rng_raw_draws"]))
    return dev, sim, gb, state


def get_stats():
    s = _lib.load().dkmc_get_stats().contents
    return {f[0]: getattr(s, f[0]) for f in s._fields_}


def get_last_X():
    """CSR of the last update_power call (dump_csr_matrix_txt twin)."""
    L = _lib.load()
    rows, nnz = C.c_int(0), C.c_longlong(0)
    check(L.dkmc_get_last_X(C.byref(rows), C.byref(nnz), None, None, None))
    rp = np.empty(rows.value + 1, dtype=np.int32); ci = np.empty(nnz.value, dtype=np.int32); data = np.empty(nnz.value)
    check(L.dkmc_get_last_X(C.byref(rows), C.byref(nnz), _np_ptr(rp), _np_ptr(ci), _np_ptr(data)))
    return rp, ci, data
