#!/usr/bin/env python3
"""Forming run gated by the filament analysis: current-off supersteps (charge, potential, KMC events) with Device.find_clusters after every
step, until a conducting cluster bridges the two contacts or the step cap is reached; then ONE superstep with the current solve.  The X solve,
which dominates a superstep, is paid only from the moment the filament has closed.
Prints one JSON line: steps run current-off, the step at which the verdict turned to bridged (null: never), gap_x after every step (null where
one of the tips does not exist), members of the analysis, and I_macro of the closing step with the current solve.
With --gaps R every check also runs Device.find_gaps at r_max = R and the line carries, per step, the bottleneck hop of the tunnelling chain and the
direct tip-to-tip gap (null: none within R): distances that close smoothly where the verdict only flips.
With --paths SLACK every check from the one whose verdict is bridged on -- that one, and the check after the closing superstep -- also runs
Device.find_paths at that slack and the line carries, per such check, the hops H of the shortest conducting path, the level and the width of the
corridor's constriction and the x range of the sites at that level.
With --track every check from the second on also runs Device.track_clusters between its labelling and the one before and the line carries, per
such check, the transition, the sites that joined, left and regrouped and the MERGED rows; the closing check also carries the number of the sites
whose arrival closed the filament and their x range.
With --cuts (needs --paths) every check that runs Device.find_paths with status 1 also runs Device.find_cuts on its path and the line carries, per
such check, the number of cut sites -- the sites whose loss alone opens the filament --, the necks as [first, last] positions and the longest
neck with its x range.
With --flow MAX every check from the one whose verdict is bridged on -- that one, and the check after the closing superstep -- also runs
Device.find_flow with max_strands = MAX and the line carries, per such check, the status, W -- the number of atoms the filament is thick at its
thinnest --, the x range of the minimum cut nearest either contact and the searches and rounds it took.
usage: python tools/run_until_bridged.py [2.5nm] [--max-steps 50] [--vd 5.0] [--members 3] [--wide-radius 0] [--gaps 0] [--paths -1] [--track]
       [--cuts] [--flow 0]"""
import argparse
import json
import math
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="2.5nm")
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--vd", type=float, default=5.0)
    ap.add_argument("--members", type=int, default=3, help="bit mask: 1 metal, 2 vacancies, 4 neutral vacancies only")
    ap.add_argument("--wide-radius", type=float, default=0.0, help="> 0: link members within this distance (gap-tolerant filament) instead of nearest neighbours")
    ap.add_argument("--gaps", type=float, default=0.0, metavar="R", help="> 0: log the bottleneck and the direct gap of Device.find_gaps(r_max=R) at every check")
    ap.add_argument("--paths", type=int, default=-1, metavar="SLACK", help=">= 0: once bridged, log H and the constriction of Device.find_paths(slack=SLACK) at every check")
    ap.add_argument("--track", action="store_true", help="from the second check on, log the transition and the joined / left / regrouped sites of Device.track_clusters")
    ap.add_argument("--cuts", action="store_true", help="with --paths: log the cut sites, the necks and the longest neck of Device.find_cuts at every check with a path")
    ap.add_argument("--flow", type=int, default=0, metavar="MAX", help="> 0: once bridged, log W and the x range of both minimum cuts of Device.find_flow(max_strands=MAX)")
    a = ap.parse_args()
    if a.cuts and a.paths < 0:
        ap.error("--cuts needs --paths")
    import torch
    from bench import Sim
    from devicekmc_amd import host
    sim = Sim(a.workload, "cuda:0", solve_current=False, Vd=a.vd)
    dev, gb, p = sim.dev, sim.gb, sim.p
    link = None
    if a.wide_radius > 0:
        wide, nn = host.build_neighbor_index_gpu(dev.site_x, dev.site_y, dev.site_z, p.lattice, p.pbc, a.wide_radius)
        link = (torch.as_tensor(wide.reshape(-1)).to("cuda:0"), nn)
    gaps, bridged_at, info = [], None, None
    bottleneck, direct = [], []
    paths, cuts = [], []

    def cut_check(step):
        _, _, _, _, necks, c = dev.find_cuts(gb, link_index=link)
        j = int((necks["first"] == c["longest_neck_first"]).argmax()) if c["necks"] else -1
        cuts.append(dict(step=step, cut_sites=c["cut_sites"], necks=[[int(f), int(l)] for f, l in zip(necks["first"], necks["last"])],
                         longest_neck=c["longest_neck"], longest_neck_first=c["longest_neck_first"],
                         longest_neck_x=[float(necks["xmin"][j]), float(necks["xmax"][j])] if j >= 0 else None,
                         bypasses=c["bypasses"], max_bypass=c["max_bypass"]))

    def path_check(step):
        _, _, _, prof, pinfo = dev.find_paths(gb, slack=a.paths, link_index=link)
        lev = pinfo["constriction_level"]
        paths.append(dict(step=step, status=pinfo["status"], hops=pinfo["hops"], constriction_level=lev, constriction_width=pinfo["constriction_width"],
                          constriction_x=[float(prof["xmin"][lev]), float(prof["xmax"][lev])] if pinfo["status"] else None,
                          corridor_sites=pinfo["corridor_sites"]))
        if a.cuts and pinfo["status"]:
            cut_check(step)

    flow = []

    def flow_check(step):
        _, _, _, _, f = dev.find_flow(gb, max_strands=a.flow, link_index=link)
        flow.append(dict(step=step, status=f["status"], width=f["width"], searches=f["searches"], rounds=f["rounds"],
                         cut_left_x=[f["cut_left_xmin"], f["cut_left_xmax"]] if f["status"] == 1 else None,
                         cut_right_x=[f["cut_right_xmin"], f["cut_right_xmax"]] if f["status"] == 1 else None))

    track = []

    def track_check(step):
        _, _, _, _, _, t = dev.track_clusters(gb)
        rec = dict(step=step, transition=host.TRACK_TRANSITION[t["transition"]], joined=t["joined"], left=t["left"], regrouped=t["regrouped"], merged=t["merged"])
        if t["transition"] == 1:
            rec.update(closing_sites=t["n_critical"], closing_x=[t["critical_xmin"], t["critical_xmax"]])
        track.append(rec)

    for k in range(a.max_steps):
        sim.step(False)
        _, _, info = dev.find_clusters(gb, members=a.members, link_index=link, capacity=0)
        if a.track and k > 0:
            track_check(k + 1)
        gaps.append(info["gap_x"] if math.isfinite(info["gap_x"]) else None)
        if a.gaps > 0:
            _, _, ginfo = dev.find_gaps(gb, r_max=a.gaps)
            bottleneck.append(ginfo["bottleneck"] if math.isfinite(ginfo["bottleneck"]) else None)
            direct.append(None if ginfo["direct"] is None else ginfo["direct"][2])
        if info["bridged"]:
            bridged_at = k + 1
            if a.paths >= 0:
                path_check(k + 1)
            if a.flow > 0:
                flow_check(k + 1)
            break
    p.solve_current = True
    sim.step(False)
    if (a.paths >= 0 or a.flow > 0) and bridged_at is not None:            # the check after the closing superstep
        _, _, after = dev.find_clusters(gb, members=a.members, link_index=link, capacity=0)
        if after["bridged"] and a.paths >= 0:
            path_check(bridged_at + 1)
        if after["bridged"] and a.flow > 0:
            flow_check(bridged_at + 1)
    more = dict(gaps_r_max=a.gaps, bottleneck=bottleneck, direct=direct) if a.gaps > 0 else {}
    if a.paths >= 0:
        more.update(paths_slack=a.paths, paths=paths)
    if a.cuts:
        more.update(cuts=cuts)
    if a.track:
        more.update(track=track)
    if a.flow > 0:
        more.update(flow_max_strands=a.flow, flow=flow)
    print(json.dumps(dict(workload=a.workload, sites=int(dev.N), Vd=a.vd, members=a.members, wide_radius=a.wide_radius, steps_current_off=len(gaps),
                          bridged_at_step=bridged_at, bridge_root=None if info is None else info["bridge_root"], gap_x=gaps,
                          n_components_last=None if info is None else info["n_components"], I_macro=dev.imacro, **more)), flush=True)
    sim.close()


if __name__ == "__main__":
    main()
