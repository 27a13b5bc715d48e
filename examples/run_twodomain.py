"""End-to-end two-domain run on the MI355X engine: clean -> split -> [item-item sim -> X-Sim extension -> AlterEgo
generation] (GPU) -> recommender sim / privacy / prediction -> MAE.

This is the build's own driver over the drop-in API (the same calls, in the same order, as the reference's
code/twodomain_demo.py:31-140, which runs unmodified against x-map_amd/ when its hard-coded
/home/tlin/notebooks paths exist -- see INTEGRATION.md).  Data: synthetic Amazon-format text files written to a
work directory (the reference ships none).

    python examples/run_twodomain.py [--users 3000] [--items 600] [--workdir /tmp/xmap_demo] [--private] [--user-based] [--device-tail [--fold-in] [--explain] [--audience] [--new-items] [--eligible] [--diverse W] [--groups K] [--peers N] [--user-knn K] [--related N] [--fill HOW] [--hybrid W] [--shelves K] [--quota C] [--calibrated] [--stock C]]

--user-based: the recommender stages with the user method of the reference's egg (calculate_xmap_sim_method = cosine_user): the
similarity between the users' AlterEgo profiles with its local sensitivity on the device (xmap.engine.session.UserSimRDD), the
neighbour selection, the user-based prediction; prints the single MAE of a user method.  The AlterEgo rows of a user who rated a
target item AND holds it through the map carry that item twice; cosine_user on the device takes profiles without repeated items,
so such rows are merged first as the reference's avoid_duplicate_ratings merges mapped ratings (the mean, the first time).

--device-tail: the recommender stages run from the AlterEgo rows in HBM to the predictions without a host conversion
(xmap.engine.session.recommend; non-private neighbour selection) and print the same MAE line.  After the MAE line: the ranking
metrics of the top-20 lists against the held-out ratings (xmap.engine.session.evaluate_topn), then the top 5 target items of
three test users (xmap.engine.session.recommend_topn).

--explain (with --device-tail): under each of those lists, why every item is there (the explain= option of recommend_topn: the
three strongest evidence entries of its score with their share, and the user's own ratings each AlterEgo row came from).

--audience (with --device-tail): the other direction -- for three target items the ten users to tell about them
(xmap.engine.session.recommend_audience: the users whose own rows give evidence for the item and who do not hold it yet, by
the same unrounded prediction).

--eligible (with --device-tail): both directions under eligibility rules -- the top 5 of the same three users over every second
target item of the catalogue ("in stock") with a score floor, without the item that led their unrestricted list ("shown
yesterday"); and the audiences of three items among every third user (a segment) above the same floor (the allow_items= /
allow_users=, exclude= and min_score= options of recommend_topn and recommend_audience: the rules act before scoring).

--diverse W (with --device-tail): the top-10 lists of the evaluated users re-ranked out of their 40 best items by greedy maximal
marginal relevance at weight W (the diversify= / pool= options of evaluate_topn and recommend_topn): NDCG@10 and the mean intra-list
similarity at weight 0 -- the plain lists -- and at W, then the re-ranked top 5 of the same three users.

--groups K (with --device-tail): one list for several users -- three groups of K members are drawn from the test users, and the top 5
of the first group are printed side by side under the three aggregates (mean, least misery, most pleasure) with the member who
likes each item least (xmap.engine.session.recommend_group: the members' unrounded predictions are aggregated on the device; a
member without evidence for an item predicts its average).

--peers N (with --device-tail): "who is this user like?" -- for three test users the N users of the train set with the most similar
AlterEgo profiles (xmap.engine.session.similar_users: centred cosine weighted by the number of common records), and each user plus
their peers as one group of recommend_group: "people like you also liked".

--user-knn K (with --device-tail): the user-based recommender beside the item-based one -- every test user's K nearest train users
(as --peers finds them), the MAE of the held-out ratings predicted from those neighbours' ratings (the reference's
user_based_prediction: xmap.engine.session.predict_user_knn), and for three test users the five items their neighbours rate highest
(recommend_user_knn; Resnick's formula, at least two neighbour ratings per item).
--related N (with --device-tail): "what goes with these items?" -- the product-page and cart query, with no user and no rating: for
three baskets drawn from held-out users' items the N items most related to the basket as a whole over the RecommenderSim rows
(xmap.engine.session.related_items: the sum of the members' similarities, the members themselves left out), and for the first
basket the list under "mean" and "max" beside it.
--fill HOW (with --device-tail; HOW = count or mean): the popularity fill -- every list is cut from candidates with evidence, so a
test user with few AlterEgo rows gets a short list and one without any an empty one.  The run prints, without and with the fill
(xmap.engine.session.recommend_topn / evaluate_topn with fill=HOW: short lists completed with the most held / best rated items
the user does not hold), the share of short lists, the share of empty lists, recall@10 and the items covered, and the head of the
ranking itself (popular_items).

--hybrid W (with --device-tail): the item-based and the user-based recommender voting together -- every test user's 64 best items
by their own rows and the 64 best items their 50 nearest users rate highest are fused on the device by reciprocal rank, the
user-based half weighted W (xmap.engine.session.recommend_hybrid: neither list leaves the device).  The run prints the ranking
metrics of the plain and of the hybrid top-10 lists side by side (evaluate_topn with hybrid=...), and for three test users the five
fused items with the half that named each.

--shelves K (with --device-tail): the front page -- not one ranking but a page of shelves, "Top picks in <category>", and the
shelves this user sees (xmap.engine.session.recommend_shelves: one device call per batch of users, no list is downloaded to be
cut).  The data carry no categories, so the items get K pseudo-categories by a hash of their id, every third item a second one.
The run prints the page of the first three test users: the four best shelves by their best item, five items each, with the size
of the whole shelf.

--quota C / --calibrated (with --device-tail): ONE list with a guaranteed mix of categories, over the pseudo-categories of --shelves
(K = 8 without it).  --quota C: at most C items of one category in a top ten, cut on the device from each test user's 256 best
candidates (xmap.engine.session.recommend_quota).  --calibrated: the ten seats go to the categories in proportion to the user's own
AlterEgo profile (mode="share": a user who only rated the other domain gets a list whose category mix follows the mapped taste).
The run prints, for the test users, how many lists changed against the plain top ten and the largest share of one category in a
list before and after.

--stock C (with --device-tail): stock limits -- every item may go to at most C of the test users (C coupons per title), every user
gets at most ten items.  The lists are cut on the device from each test user's 64 best candidates by deferred acceptance over all
the test users at once (xmap.engine.session.recommend_allotted): an item keeps its C best offers by score, a user moves down its
pool past the items that refused it.  The run prints how many lists changed against the plain top ten, the seats filled, the rounds
and the share of users left short of ten.

--new-items (with --device-tail): three target items are kept out of training altogether, as items that enter the catalogue
afterwards would be.  The model is trained without them; the ratings they collected in the training period are then folded in
(xmap.engine.session.recommend_audience_items / recommend_items: one row of RecommenderSim per item against the frozen AlterEgo
profiles, the model unchanged), and the run prints their neighbour lists' lengths, their audiences and the MAE of their
held-out ratings.

--fold-in (with --device-tail): five test users are kept out of training altogether, as users who arrive afterwards would be.
The model is trained without them; their ratings (the source domain's, for a user known only there) are then folded in
(xmap.engine.session.recommend_topn_profiles / recommend_profiles: AlterEgo profiles from the resident replacement map, the
model unchanged), and the run prints their top 5 target items and the MAE of their held-out target ratings.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x-map_amd"))

import yaml  # noqa: E402
from pyspark import SparkContext, SparkConf  # noqa: E402
from pyspark.sql import SQLContext  # noqa: E402

from xmap.core.baselinerClean import BaselinerClean  # noqa: E402
from xmap.core.baselinerSplit import BaselinerSplit  # noqa: E402
from xmap.core.baselinerSim import BaselinerSim  # noqa: E402
from xmap.core.extender import ExtendSim  # noqa: E402
from xmap.core.generator import Generator  # noqa: E402
from xmap.core.recommenderSim import RecommenderSim  # noqa: E402
from xmap.core.recommenderPrivacy import RecommenderPrivacy  # noqa: E402
from xmap.core.recommenderPrediction import RecommenderPrediction  # noqa: E402
from xmap.utils import assist  # noqa: E402
from xmap.engine import synth  # noqa: E402


def write_inputs(workdir, users, items, seed):
    """book.txt (source) / movie.txt (target) in `uid \\t iid \\t rating \\t unix_ts` + parameters.yaml"""
    raw = os.path.join(workdir, "data", "raw")
    os.makedirs(raw, exist_ok=True)
    r = synth.make_two_domain(seed, users, items, items, overlap=0.35)
    with open(os.path.join(raw, "book.txt"), "w") as fb, open(os.path.join(raw, "movie.txt"), "w") as fm:
        for u in range(r.n_users):
            for e in range(r.user_ptr[u], r.user_ptr[u + 1]):
                it = int(r.item[e])
                src = it < r.n_src_items
                rid = "%010d" % r.src_numbers[it] if src else "B0%08d" % r.tgt_numbers[it - r.n_src_items]
                (fb if src else fm).write("A%013d\t%s\t%.1f\t%d\n" % (u, rid, float(r.rating[e]), int(r.time[e])))
    para = {
        "init": {"path_hdfs": "file:" + os.path.join(workdir, "data"), "path_movie": "raw/movie.txt",
                 "path_book": "raw/book.txt", "is_debug": False, "seed": 666666, "num_partition": 30},
        "baseliner": {"num_atleast_rating": 5, "size_subset": 6666, "date_from": 2012, "date_to": 2013, "num_left": 0,
                      "ratio_split": 0.2, "ratio_both": 0.8, "calculate_baseline_sim_method": "adjust_cosine",
                      "calculate_baseline_weighting": 50},
        "extender": {"extend_among_topk": 10},
        "generator": {"private_flag": False, "mapping_range": 1, "private_epsilon": 0.6, "private_rpo": 0.1},
        "recommender": {"calculate_xmap_sim_method": "cosine_item", "calculate_xmap_weighting": 50, "mapping_range": 10,
                        "private_flag": False, "private_epsilon": 0.6, "private_rpo": 0.1, "decay_alpha": 0.03},
    }
    path = os.path.join(workdir, "parameters.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(para, f)
    return path


def merge_repeated_items(sc, alterEgo_profile):
    """(uid, iid, rating, time) rows with one row per (uid, iid): the mean rating and the first time of the rows that meet"""
    import numpy as np
    merged = {}
    for uid, iid, rating, when in alterEgo_profile.collect():
        merged.setdefault((uid, iid), []).append((rating, when))
    return sc.parallelize([(uid, iid, float(np.mean([r for r, _ in v])), v[0][1]) for (uid, iid), v in merged.items()])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=3000)
    ap.add_argument("--items", type=int, default=600)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--workdir", default="/tmp/xmap_demo")
    ap.add_argument("--private", action="store_true")
    ap.add_argument("--user-based", action="store_true")
    ap.add_argument("--device-tail", action="store_true")
    ap.add_argument("--fold-in", action="store_true")
    ap.add_argument("--explain", action="store_true")
    ap.add_argument("--audience", action="store_true")
    ap.add_argument("--new-items", action="store_true")
    ap.add_argument("--eligible", action="store_true")
    ap.add_argument("--diverse", type=float, default=None, metavar="W")
    ap.add_argument("--groups", type=int, default=None, metavar="K")
    ap.add_argument("--peers", type=int, default=None, metavar="N")
    ap.add_argument("--user-knn", type=int, default=None, metavar="K")
    ap.add_argument("--related", type=int, default=None, metavar="N")
    ap.add_argument("--fill", default=None, choices=["count", "mean"], metavar="HOW")
    ap.add_argument("--hybrid", type=float, default=None, metavar="W")
    ap.add_argument("--shelves", type=int, default=None, metavar="K")
    ap.add_argument("--quota", type=int, default=None, metavar="C")
    ap.add_argument("--calibrated", action="store_true")
    ap.add_argument("--stock", type=int, default=None, metavar="C")
    args = ap.parse_args(argv)
    para = assist.load_parameter(write_inputs(args.workdir, args.users, args.items, args.seed))
    if args.private:
        para["generator"]["private_flag"] = True
        para["recommender"]["private_flag"] = True
    if args.user_based:
        if args.device_tail:
            ap.error("--user-based runs the reference pipeline; --device-tail is the item-based tail")
        para["recommender"]["calculate_xmap_sim_method"] = "cosine_user"
    sc = SparkContext(conf=SparkConf().setAppName("xmap two-domain on MI355X"))
    sqlContext = SQLContext(sc)
    b, g, rc = para["baseliner"], para["generator"], para["recommender"]
    t = {}

    def timed(name, f, *a, **kw):
        t0 = time.time()
        out = f(*a, **kw)
        t[name] = time.time() - t0
        return out
    clean_s = BaselinerClean(b["num_atleast_rating"], b["size_subset"], b["date_from"], b["date_to"], domain_label="S:")
    clean_t = BaselinerClean(b["num_atleast_rating"], b["size_subset"], b["date_from"], b["date_to"], domain_label="T:")
    split = BaselinerSplit(b["num_left"], b["ratio_split"], b["ratio_both"], para["init"]["seed"])
    sim_tool = BaselinerSim(b["calculate_baseline_sim_method"], b["calculate_baseline_weighting"])
    hdfs = para["init"]["path_hdfs"]
    sourceRDD = timed("clean_source", assist.baseliner_clean_data_pipeline, sc, clean_s,
                      os.path.join(hdfs, para["init"]["path_book"]), para["init"]["is_debug"], para["init"]["num_partition"])
    targetRDD = timed("clean_target", assist.baseliner_clean_data_pipeline, sc, clean_t,
                      os.path.join(hdfs, para["init"]["path_movie"]), para["init"]["is_debug"], para["init"]["num_partition"])
    trainRDD, testRDD = timed("split", assist.baseliner_split_data_pipeline, sc, split, sourceRDD, targetRDD)
    if args.audience and (not args.device_tail or para["recommender"]["private_flag"]):
        ap.error("--audience needs --device-tail and the non-private recommender")
    if args.eligible and (not args.device_tail or para["recommender"]["private_flag"]):
        ap.error("--eligible needs --device-tail and the non-private recommender")
    if args.diverse is not None and (not args.device_tail or para["recommender"]["private_flag"]):
        ap.error("--diverse needs --device-tail and the non-private recommender")
    if args.groups is not None and (not args.device_tail or para["recommender"]["private_flag"] or not 1 <= args.groups <= 64):
        ap.error("--groups K needs --device-tail, the non-private recommender and 1 <= K <= 64")
    if args.user_knn is not None and (not args.device_tail or para["recommender"]["private_flag"] or not 1 <= args.user_knn <= 1024):
        ap.error("--user-knn K needs --device-tail, the non-private recommender and 1 <= K <= 1024")
    if args.related is not None and (not args.device_tail or not 1 <= args.related <= 1024):
        ap.error("--related N needs --device-tail and 1 <= N <= 1024")
    if args.fill is not None and (not args.device_tail or para["recommender"]["private_flag"]):
        ap.error("--fill HOW needs --device-tail and the non-private recommender")
    if args.hybrid is not None and (not args.device_tail or para["recommender"]["private_flag"] or not 0.0 <= args.hybrid < float("inf")):
        ap.error("--hybrid W needs --device-tail, the non-private recommender and a finite W >= 0")
    if args.shelves is not None and (not args.device_tail or para["recommender"]["private_flag"] or not 1 <= args.shelves <= 1000):
        ap.error("--shelves K needs --device-tail, the non-private recommender and 1 <= K <= 1000")
    if (args.quota is not None or args.calibrated) and (not args.device_tail or para["recommender"]["private_flag"] or
                                                        (args.quota is not None and args.quota < 1)):
        ap.error("--quota C and --calibrated need --device-tail, the non-private recommender and C >= 1")
    if args.stock is not None and (not args.device_tail or para["recommender"]["private_flag"] or args.stock < 1):
        ap.error("--stock C needs --device-tail, the non-private recommender and C >= 1")
    if args.peers is not None and (not args.device_tail or para["recommender"]["private_flag"] or not 1 <= args.peers <= 63):
        ap.error("--peers N needs --device-tail, the non-private recommender and 1 <= N <= 63")
    late = []                   # (uid, profile) of the users who arrive after training
    if args.fold_in:
        if not args.device_tail or para["recommender"]["private_flag"]:
            ap.error("--fold-in needs --device-tail and the non-private recommender")
        late_uids = set(uid for uid, _ in testRDD.take(5))
        late = trainRDD.filter(lambda rec: rec[0] in late_uids).collect()
        trainRDD = trainRDD.filter(lambda rec: rec[0] not in late_uids).cache()
    new_items = []              # (iid, [(uid, rating)*]) of the items that enter the catalogue after training
    if args.new_items:
        if not args.device_tail or para["recommender"]["private_flag"]:
            ap.error("--new-items needs --device-tail and the non-private recommender")
        raters = {}
        for uid, prof in trainRDD.collect():
            for entry in prof:
                if "T:" in entry[0]:
                    raters.setdefault(entry[0], []).append((uid, entry[1]))
        new_iids = set(sorted(raters, key=lambda iid: (- len(raters[iid]), iid))[10:13])      # well rated, not the very heaviest
        new_items = [(iid, raters[iid]) for iid in sorted(new_iids)]
        trainRDD = trainRDD.map(lambda rec: (rec[0], [e for e in rec[1] if e[0] not in new_iids])).filter(lambda rec: rec[1]).cache()
    item2item_simRDD = timed("A_item_sim", assist.baseliner_calculate_sim_pipeline, sc, sim_tool, trainRDD)
    ext_tool = ExtendSim(para["extender"]["extend_among_topk"])
    extendedsimRDD = timed("B_extend", assist.extender_pipeline, sc, sqlContext, sim_tool, ext_tool, item2item_simRDD)
    gen_tool = Generator(g["mapping_range"], g["private_epsilon"], b["calculate_baseline_sim_method"], g["private_rpo"])
    alterEgo_profile = timed("C_generate", assist.generator_pipeline, gen_tool, trainRDD, extendedsimRDD, g["private_flag"])
    rsim = RecommenderSim(rc["calculate_xmap_sim_method"], rc["calculate_xmap_weighting"])
    rpriv = RecommenderPrivacy(rc["mapping_range"], rc["private_epsilon"], rc["private_rpo"])
    rpred = RecommenderPrediction(rc["decay_alpha"], rc["calculate_xmap_sim_method"])
    if args.device_tail and not rc["private_flag"]:
        from xmap.engine import session
        predicted = timed("recommender_device_tail", session.recommend, alterEgo_profile, testRDD, rc["calculate_xmap_weighting"],
                          rc["mapping_range"], rc["decay_alpha"])
        mae = rpred.calculate_mae(predicted)
    else:
        profile = merge_repeated_items(sc, alterEgo_profile) if args.user_based else alterEgo_profile
        _, _, ubd, ibd, uinfo, iinfo, alterEgo_sim = timed(
            "recommender_sim", assist.recommender_calculate_sim_pipeline, sc, rsim, profile)
        kept = timed("recommender_privacy", assist.recommender_privacy_pipeline, rpriv, alterEgo_sim, rc["private_flag"])
        simpair_bd = sc.broadcast(kept.collectAsMap())
        mae = timed("recommender_prediction", assist.recommender_prediction_pipeline, rpred, rsim, testRDD, simpair_bd,
                    ubd, ibd, uinfo, iinfo)
    assist.write_to_disk({"mae": mae}, para, os.path.join(args.workdir, "data", "output"))
    sc.stop()
    print("train users %d, test users %d, sim pairs %d, AlterEgo rows %d" % (
        trainRDD.count(), testRDD.count(), item2item_simRDD.count(), alterEgo_profile.count()))
    if args.user_based:
        print("MAE (user-based):", mae)
        return mae
    print("MAE (no decay; decay):", mae)
    from xmap.engine import session
    if isinstance(alterEgo_profile, session.AlterEgoRDD) and not rc["private_flag"]:
        # the ranking quality of the lists against the held-out ratings (relevant: 4 stars and more), scored on the device
        ev = session.evaluate_topn(alterEgo_profile, testRDD, rc["calculate_xmap_weighting"], rc["mapping_range"], rc["decay_alpha"], 20,
                                   cutoffs=(5, 10, 20), rel_min=4.0)
        for c in sorted(ev.at):
            m = ev.at[c]
            print("top-%d over %d users: hit rate %.4f, precision %.4f, recall %.4f, NDCG %.4f, MAP %.4f, MRR %.4f, %d items covered" % (
                c, m["users"], m["hit_rate"], m["precision"], m["recall"], m["ndcg"], m["map"], m["mrr"], m["coverage"]))
        # what the library is for: target-domain items for users known through their source-domain ratings
        top = session.recommend_topn(alterEgo_profile, [uid for uid, _ in testRDD.take(3)], rc["calculate_xmap_weighting"],
                                     rc["mapping_range"], rc["decay_alpha"], 5, explain=(3, 4) if args.explain else None)
        for q, (uid, lst) in enumerate(top.collect()):
            print("top 5 for %s:" % uid, ", ".join("%s (%.3f)" % (iid, plain) for iid, plain, _ in lst) or "no evidence")
            for iid, entries in (top.explanations[q][1] if args.explain else []):
                print("  %s, because of" % iid)
                for nid, s, rating, share, sources, n_all in entries:
                    cited = ", ".join("%s rated %s" % (sid, sr) for sid, sr, _ in sources) + (", ..." if n_all > len(sources) else "")
                    print("    %+.3f  %s (similarity %.3f, your AlterEgo rating %.2f)  <-  %s" % (share, nid, s, rating, cited))
    if args.audience:
        # the other direction: whom to tell about an item (here: the first three items that have a neighbour list)
        aud = timed("audience", session.recommend_audience, alterEgo_profile, sorted(top.sim_pairs)[:3], rc["calculate_xmap_weighting"],
                    rc["mapping_range"], rc["decay_alpha"], 10)
        for iid, lst in aud.collect():
            print("audience of %s:" % iid, ", ".join("%s (%.3f)" % (uid, plain) for uid, plain, _ in lst) or "no evidence")
    if args.eligible:
        # the same two calls under eligibility rules: a catalogue subset, yesterday's item, a segment, a floor
        w, k, alpha = rc["calculate_xmap_weighting"], rc["mapping_range"], rc["decay_alpha"]
        in_stock = sorted(top.sim_pairs)[::2]
        shown = {uid: [lst[0][0]] for uid, lst in top.collect() if lst}
        floor = 3.0
        el = timed("eligible_topn", session.recommend_topn, alterEgo_profile, [uid for uid, _ in top.collect()], w, k, alpha, 5,
                   allow_items=in_stock, exclude=shown, min_score=floor)
        print("eligible: %d of %d listed items in stock, floor %.1f: %d pairs scored, %d removed before scoring, %d below the floor" % (
            len(in_stock), len(top.sim_pairs), floor, el.stats[0], el.stats[5], el.stats[4]))
        for uid, lst in el.collect():
            print("eligible top 5 for %s:" % uid, ", ".join("%s (%.3f)" % (iid, plain) for iid, plain, _ in lst) or "nothing eligible")
        segment = trainRDD.map(lambda rec: rec[0]).collect()[::3]
        el = timed("eligible_audience", session.recommend_audience, alterEgo_profile, in_stock[:3], w, k, alpha, 10,
                   allow_users=segment, min_score=floor)
        print("eligible: a segment of %d users: %d pairs scored, %d removed before scoring, %d below the floor" % (
            len(segment), el.stats[0], el.stats[5], el.stats[4]))
        for iid, lst in el.collect():
            print("eligible audience of %s:" % iid, ", ".join("%s (%.3f)" % (uid, plain) for uid, plain, _ in lst) or "nobody eligible")
    if args.diverse is not None:
        # score against redundancy: the same evaluation over lists re-ranked out of a pool of 40, at weight 0 and at W
        w, k, alpha = rc["calculate_xmap_weighting"], rc["mapping_range"], rc["decay_alpha"]
        for weight in (0.0, args.diverse):
            ev = timed("diverse_eval_w%g" % weight, session.evaluate_topn, alterEgo_profile, testRDD, w, k, alpha, 10, cutoffs=(10,),
                       rel_min=4.0, diversify=weight, pool=40)
            print("diversify %g: NDCG@10 %.4f, mean intra-list similarity %.4f, %d items covered, over %d users" % (
                weight, ev.at[10]["ndcg"], ev.ils, ev.at[10]["coverage"], ev.at[10]["users"]))
        dv = timed("diverse_topn", session.recommend_topn, alterEgo_profile, [uid for uid, _ in top.collect()], w, k, alpha, 5,
                   diversify=args.diverse, pool=40)
        for (uid, lst), ils in zip(dv.collect(), dv.ils):
            print("diversified top 5 for %s (intra-list similarity %.3f):" % (uid, ils),
                  ", ".join("%s (%.3f)" % (iid, plain) for iid, plain, _ in lst) or "no evidence")
    if args.groups is not None:
        # one list for several users: K-member groups of test users under the three aggregates
        w, k, alpha = rc["calculate_xmap_weighting"], rc["mapping_range"], rc["decay_alpha"]
        pool = [uid for uid, _ in testRDD.take(3 * args.groups)]
        parties = [("group %d" % (g + 1), pool[g * args.groups:(g + 1) * args.groups]) for g in range(3) if pool[g * args.groups:(g + 1) * args.groups]]
        by_how = {}
        for how in ("mean", "min", "max"):
            by_how[how] = timed("group_topn_" + how, session.recommend_group, alterEgo_profile, parties, w, k, alpha, 5, how=how)
        st = by_how["mean"].stats
        print("groups: %d of %d members: %d member pairs scored, %d group candidates (largest group %d)" % (
            len(parties), args.groups, st[0], st[7], st[3]))
        gid, members = parties[0]
        print("%s = %s" % (gid, ", ".join(members)))
        print("  %-44s | %-44s | %-44s" % ("mean", "least misery", "most pleasure"))
        cols = [by_how[how].collect()[0][1] for how in ("mean", "min", "max")]
        for pos in range(max(len(c) for c in cols)):
            print("  " + " | ".join("%-44s" % ("%s %.3f (least: %s)" % (c[pos][0], c[pos][1], c[pos][3]) if pos < len(c) else "") for c in cols))
    if args.peers is not None:
        # who is this user like?  The N nearest profiles of a few test users, then each user and their peers as ONE group:
        # "people like you also liked"
        w, k, alpha = rc["calculate_xmap_weighting"], rc["mapping_range"], rc["decay_alpha"]
        some = [uid for uid, _ in testRDD.take(3)]
        peers = timed("similar_users", session.similar_users, alterEgo_profile, some, args.peers, cap=5, min_common=2)
        print("peers: %d candidates of %d users, %d records expanded (largest candidate count %d)" % (
            peers.stats[0], len(some), peers.stats[5], peers.stats[4]))
        for uid, lst in peers.collect():
            print("peers of %s:" % uid, ", ".join("%s (%.3f, %d in common)" % e for e in lst) or "nobody shares an item")
        circles = [("%s and peers" % uid, [uid] + [u2 for u2, _, _ in lst]) for uid, lst in peers.collect()]
        liked = timed("peers_group_topn", session.recommend_group, alterEgo_profile, circles, w, k, alpha, 5, how="mean")
        for gid, lst in liked.collect():
            print("people like you also liked (%s):" % gid, ", ".join("%s (%.3f)" % (iid, plain) for iid, plain, _, _ in lst) or "no evidence")
    if args.user_knn is not None:
        # the user-based recommender: predictions and lists from the ratings of the K nearest users
        ub, ub_mae = timed("user_knn_predict", session.predict_user_knn, alterEgo_profile, testRDD, args.user_knn, cap=5, min_common=2)
        print("user-kNN (K = %d): MAE %s over %d of %d held-out pairs" % (
            args.user_knn, ub_mae, int(ub.mae[0]) if ub.mae else 0, sum(len(p) for _, p in testRDD.collect())))
        some = [uid for uid, _ in testRDD.take(3)]
        lists = timed("user_knn_topn", session.recommend_user_knn, alterEgo_profile, some, args.user_knn, 5, cap=5, min_common=2,
                      own_mean=True, min_support=2)
        print("user-kNN lists: %d candidates of %d users, %d records expanded" % (lists.stats[0], len(some), lists.stats[5]))
        for uid, lst in lists.collect():
            print("people like %s rated highly:" % uid, ", ".join("%s (%.3f, %d ratings)" % e for e in lst) or "no neighbour rated anything new")
    if args.related is not None:
        # what goes with these items?  Baskets of a few held-out items each: no user, no rating
        carts = [("basket of %s" % uid, [e[0] for e in pairs[:3]]) for uid, pairs in testRDD.take(3)]
        by_how = {}
        for how in ("sum", "mean", "max"):
            by_how[how] = timed("related_" + how, session.related_items, alterEgo_profile, carts, rc["calculate_xmap_weighting"], args.related,
                                how=how)
        rel = by_how["sum"]
        print("related: %d candidates of %d baskets, %d records expanded (largest candidate count %d), %d unknown members" % (
            rel.stats[0], len(carts), rel.stats[5], rel.stats[4], rel.unknown_items))
        for (label, members), (_, lst) in zip(carts, rel.collect()):
            print("%s = %s" % (label, ", ".join(members)))
            print("  goes with:", ", ".join("%s (%.3f, %d of %d)" % (iid, s, n, len(members)) for iid, s, n in lst) or "nothing related")
        for how in ("mean", "max"):
            print("  first basket by %s:" % how, ", ".join("%s (%.3f)" % (iid, s) for iid, s, _ in by_how[how].collect()[0][1]) or "nothing related")
    if args.fill is not None:
        # what the fill buys: the lists of every test user without and with it, scored against the held-out ratings
        w, k, alpha = rc["calculate_xmap_weighting"], rc["mapping_range"], rc["decay_alpha"]
        spec = args.fill if args.fill == "count" else dict(how="mean", damping=25.0, min_count=2)
        everyone = [uid for uid, _ in testRDD.collect()]
        print("fill = %s: %d test users, lists of 10" % (args.fill, len(everyone)))
        print("  %-8s %12s %12s %10s %10s" % ("", "short lists", "empty lists", "recall@10", "coverage"))
        for name, fill in (("without", None), ("with", spec)):
            lists = timed("topn_fill_" + name, session.recommend_topn, alterEgo_profile, everyone, w, k, alpha, 10, fill=fill).collect()
            ev = session.evaluate_topn(alterEgo_profile, testRDD, w, k, alpha, 10, cutoffs=(10,), rel_min=4.0, fill=fill)
            print("  %-8s %11.1f%% %11.1f%% %10.4f %10d" % (
                name, 100.0 * sum(len(l) < 10 for _, l in lists) / max(len(lists), 1),
                100.0 * sum(not l for _, l in lists) / max(len(lists), 1), ev.at[10]["recall"], ev.at[10]["coverage"]))
        shelf = session.popular_items(alterEgo_profile, w, 5, **(dict(how="count") if args.fill == "count" else spec))
        print("  the shelf of an anonymous visitor:", ", ".join("%s (%.3f)" % e for e in shelf))
    if args.hybrid is not None:
        # the item-based and the user-based lists fused on the device: what the vote of the two buys, and who named what
        w, k, alpha = rc["calculate_xmap_weighting"], rc["mapping_range"], rc["decay_alpha"]
        hyb = dict(n_nb=50, peer_cap=5, min_common=2, own_mean=True, how="rrf", weights=(1.0, args.hybrid))
        print("hybrid (RRF, user-based half weighted %g): lists of 10" % args.hybrid)
        print("  %-8s %10s %10s %10s %10s %10s" % ("", "hit rate", "recall@10", "NDCG@10", "MAP", "coverage"))
        for name, spec in (("plain", None), ("hybrid", hyb)):
            ev = timed("hybrid_eval_" + name, session.evaluate_topn, alterEgo_profile, testRDD, w, k, alpha, 10, cutoffs=(10,), rel_min=4.0,
                       hybrid=spec)
            m = ev.at[10]
            print("  %-8s %10.4f %10.4f %10.4f %10.4f %10d" % (name, m["hit_rate"], m["recall"], m["ndcg"], m["map"], m["coverage"]))
        fused = timed("hybrid_topn", session.recommend_hybrid, alterEgo_profile, [uid for uid, _ in testRDD.take(3)], w, k, alpha, 5,
                      hyb["n_nb"], **{key: v for key, v in hyb.items() if key != "n_nb"})
        print("  %d candidates of %d records; %d item-based and %d user-based candidates went in" % (
            fused.stats[2][0], fused.stats[2][4], fused.stats[0][0], fused.stats[1][0]))
        for uid, lst in fused.collect():
            print("hybrid top 5 for %s:" % uid, ", ".join("%s (%.4f, %s)" % (iid, s, "+".join(which)) for iid, s, which in lst) or "no evidence")
    if args.shelves is not None or args.quota is not None or args.calibrated:
        # pseudo-categories by a hash of the iid, every third item carries a second one
        import zlib
        w, k, alpha = rc["calculate_xmap_weighting"], rc["mapping_range"], rc["decay_alpha"]
        K = args.shelves if args.shelves is not None else 8
        iids = trainRDD.flatMap(lambda rec: [e[0] for e in rec[1]]).distinct().collect()
        cats = {}
        for iid in iids:
            h = zlib.crc32(iid.encode())
            cats[iid] = ["category %03d" % (h % K)] + (["category %03d" % ((h // 7) % K)] if h % 3 == 0 else [])
    if args.quota is not None or args.calibrated:
        # one list with a guaranteed mix: caps per category, or seats in proportion to the user's own profile
        test_uids = [uid for uid, _ in testRDD.collect()]
        plain = timed("plain_top10", session.recommend_topn, alterEgo_profile, test_uids, w, k, alpha, 10).collect()

        def largest_share(lists):
            shares = []
            for _, lst in lists:
                seen = {}
                for e in lst:
                    for c in set(cats.get(e[0], ())):
                        seen[c] = seen.get(c, 0) + 1
                if lst:
                    shares.append(max(seen.values()) / float(len(lst)) if seen else 0.0)
            return (sum(shares) / len(shares), max(shares)) if shares else (0.0, 0.0)

        runs = ([("quota %d" % args.quota, dict(at_most=args.quota))] if args.quota is not None else []) + \
               ([("calibrated", dict(mode="share"))] if args.calibrated else [])
        for name, kw in runs:
            out = timed(name.split()[0], session.recommend_quota, alterEgo_profile, test_uids, w, k, alpha, cats, 10, 256, **kw)
            before, after = largest_share(plain), largest_share(out.collect())
            print("%s: %d of %d lists changed; the largest share of one category in a list: mean %.2f -> %.2f, worst %.2f -> %.2f%s" % (
                name, out.stats[6], len(test_uids), before[0], after[0], before[1], after[1],
                "; %d lists cut short by the pool of 256" % out.cut_short if out.cut_short else ""))
    if args.stock is not None:
        # stock limits: every item goes to at most C of the test users -- one market over all of them
        w, k, alpha = rc["calculate_xmap_weighting"], rc["mapping_range"], rc["decay_alpha"]
        test_uids = [uid for uid, _ in testRDD.collect()]
        out = timed("allotted", session.recommend_allotted, alterEgo_profile, test_uids, w, k, alpha, 10, 64, stock=args.stock)
        lists = out.collect()
        seats, short = sum(len(lst) for _, lst in lists), sum(1 for _, lst in lists if len(lst) < 10)
        print("stock %d: %d of %d lists changed; %d seats filled over %d items (the fullest holds %d); %d rounds, %d offers refused; "
              "%.1f %% of the users left short of ten%s" % (
                  args.stock, out.changed, len(test_uids), seats, len(out.taken), max(out.taken.values()) if out.taken else 0, out.rounds,
                  out.stats[8], 100.0 * short / max(len(test_uids), 1),
                  "; %d lists cut short by the pool of 64" % out.cut_short if out.cut_short else ""))
    if args.shelves is not None:
        # a page of shelves per user
        page = timed("shelves", session.recommend_shelves, alterEgo_profile, [uid for uid, _ in testRDD.take(3)], w, k, alpha, cats, 4, 5)
        print("shelves: %d labels, %d (candidate, label) records, %d shelves with a member, at most %d for one user" % (
            len(page.label_names), page.stats[6], page.stats[7], page.stats[9]))
        for uid, shelves in page.collect():
            print("the page of %s:" % uid if shelves else "the page of %s: no evidence" % uid)
            for name, score, size, lst in shelves:
                print("  top picks in %s (%d of %d):" % (name, len(lst), size), ", ".join("%s (%.3f)" % e for e in lst))
    if new_items:
        w, k, alpha = rc["calculate_xmap_weighting"], rc["mapping_range"], rc["decay_alpha"]
        aud = timed("item_fold_in_audience", session.recommend_audience_items, alterEgo_profile, new_items, w, k, alpha, 10)
        print("item fold-in: %d items kept out of training, %d ratings -> %d records, %d pairs, %d unknown users" % (
            len(new_items), sum(len(l) for _, l in new_items), aud.counts[1], aud.counts[0], aud.unknown_users))
        for iid, lst in aud.collect():
            print("audience of %s (folded in, %d neighbours):" % (iid, len(aud.new_sim_pairs.get(iid, ()))),
                  ", ".join("%s (%.3f)" % (uid, plain) for uid, plain, _ in lst) or "no evidence")
        names = set(iid for iid, _ in new_items)
        held = testRDD.map(lambda rec: (rec[0], [e for e in rec[1] if e[0] in names])).filter(lambda rec: rec[1])
        print("MAE of their held-out ratings (no decay; decay):",
              rpred.calculate_mae(session.recommend_items(alterEgo_profile, new_items, held, w, k, alpha)))
    if late:
        w, k, alpha = rc["calculate_xmap_weighting"], rc["mapping_range"], rc["decay_alpha"]
        top = timed("fold_in_topn", session.recommend_topn_profiles, alterEgo_profile, late, w, k, alpha, 5)
        print("fold-in: %d users kept out of training, %d ratings -> %d AlterEgo rows (%d pass-through), %d unknown items" % (
            len(late), sum(len(p) for _, p in late), top.counts[0], top.counts[1], top.unknown_items))
        for uid, lst in top.collect():
            print("top 5 for %s (folded in):" % uid, ", ".join("%s (%.3f)" % (iid, plain) for iid, plain, _ in lst) or "no evidence")
        held = testRDD.filter(lambda rec: rec[0] in late_uids)
        print("MAE of their held-out target ratings (no decay; decay):",
              rpred.calculate_mae(session.recommend_profiles(alterEgo_profile, late, held, w, k, alpha)))
    print("seconds:", {k: round(v, 3) for k, v in t.items()})
    return mae


if __name__ == "__main__":
    main()
