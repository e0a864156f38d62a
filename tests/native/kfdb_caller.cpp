/* kfdb_caller.cpp — Planar_SLAM::KeyFrameDatabase of include/drfe_adaptor.hpp driven as LoopClosing::DetectLoop and
 * Tracking::Relocalization drive the reference's (src/LoopClosing.cc:127-167, src/Tracking.cc:3550), on stand-in key frames and
 * frames: add -> a loop query -> erase -> a loop and a relocalisation query -> add again -> the two batch forms.
 *
 *   kfdb_caller [host | device]
 *
 * Every candidate list is compared with one worked out by hand.  All values are powers of two; for positive values a common word
 * adds min(vi, wi) to the score, so against a query of four words of 0.25 a key frame with the same words at 0.125 scores 0.5 and
 * one equal to the query 1.0:
 *   key frames 10 and 11 score 0.5 and have 12 (1.0) as their one covisibility neighbour.
 *   1. 10, 11, 12 added; loop query of key frame 1: 10 and 11 reach 1.5 and elect 12, 12 stays at 1.0 < 0.75 * 1.5  -> {12}
 *   2. 12 erased; loop query of key frame 2: 10 and 11 at 0.5, their neighbour is in no list                       -> {10, 11}
 *   3. relocalisation of frame 1 (the same words): the same, nothing stale is read                                  -> {10, 11}
 *   4. 12 added again (now last in every word's list); relocalisation of frame 2                                    -> {12}
 *   5. the queue {3, 4} with add after each: 3 is connected to and covisible with 10 (minScore 0.5): 11 elects 12 -> {12};
 *      4 is connected to and covisible with 3, by then in the inverted file (minScore 1.0): only 12 reaches it      -> {12}
 *   6. frames {3, 4} in one call.  Frame 3 now also meets key frames 3 and 4 (1.0 each): 10 and 11 reach 1.5, 12 1.0, 3 adds its
 *      neighbour 10 (1.5), 4 adds its neighbour 3 (2.0, not above its own 1.0: it elects itself); only 2.0 > 0.75 * 2.0 -> {4};
 *      frame 4 shares no word -> {}
 *   7. clear(); loop query of key frame 5 -> {} */
#include "drfe_adaptor.hpp"

#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace {

struct KeyFrame {
    long unsigned int mnId = 0;
    std::map<unsigned int, double> mBowVec;
    bool mbBad = false;
    std::set<KeyFrame*> mConnected;
    std::vector<KeyFrame*> mOrdered;                 /* by weight, best first */
    bool isBad() const { return mbBad; }
    std::set<KeyFrame*> GetConnectedKeyFrames() const { return mConnected; }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() const { return mOrdered; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) const
    {
        return (int)mOrdered.size() < N ? mOrdered : std::vector<KeyFrame*>(mOrdered.begin(), mOrdered.begin() + N);
    }
};

struct Frame {
    long unsigned int mnId = 0;
    std::map<unsigned int, double> mBowVec;
};

using Database = Planar_SLAM::KeyFrameDatabase<KeyFrame, Frame>;

std::map<unsigned int, double> words(double v, unsigned int first = 1)
{
    std::map<unsigned int, double> m;
    for (unsigned int w = first; w < first + 4; w++) m[w] = v;
    return m;
}

int failures = 0;

void expect(const char* what, const std::vector<KeyFrame*>& got, const std::vector<long unsigned int>& want)
{
    bool same = got.size() == want.size();
    for (size_t i = 0; same && i < got.size(); i++) same = got[i]->mnId == want[i];
    if (same) return;
    failures++;
    fprintf(stderr, "kfdb_caller: %s: got {", what);
    for (KeyFrame* k : got) fprintf(stderr, " %lu", k->mnId);
    fprintf(stderr, " }\n");
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "host";
    try {
        struct Vocabulary {} voc;
        Database db(voc, mode == "device" ? 0 : -1);
        db.UseDevice(mode == "device");
        std::map<int, KeyFrame> kf;
        for (int id : {1, 2, 3, 4, 5, 10, 11, 12}) {
            kf[id].mnId = (long unsigned int)id;
            kf[id].mBowVec = words(id == 10 || id == 11 ? 0.125 : 0.25);
        }
        kf[10].mOrdered = {&kf[12]};
        kf[11].mOrdered = {&kf[12]};
        for (int id : {10, 11, 12}) db.add(&kf[id]);
        expect("1 loop query", db.DetectLoopCandidates(&kf[1], 0.0f), {12});
        db.erase(&kf[12]);
        db.erase(&kf[12]);                                     /* not in the inverted file any more: left alone */
        expect("2 loop query after erase", db.DetectLoopCandidates(&kf[2], 0.0f), {10, 11});
        Frame f[5];
        for (int i = 1; i <= 4; i++) {
            f[i].mnId = (long unsigned int)i;
            f[i].mBowVec = words(0.25, i == 4 ? 50 : 1);
        }
        expect("3 relocalisation after erase", db.DetectRelocalizationCandidates(&f[1]), {10, 11});
        if (db.UninitReads() != std::vector<int32_t>{0}) { failures++; fprintf(stderr, "kfdb_caller: 3: an uninitialised read\n"); }
        db.add(&kf[12]);
        expect("4 relocalisation after add", db.DetectRelocalizationCandidates(&f[2]), {12});
        kf[3].mConnected = {&kf[10]};
        kf[3].mOrdered = {&kf[10]};
        kf[4].mConnected = {&kf[3]};
        kf[4].mOrdered = {&kf[3]};
        const auto queued = db.DetectLoopCandidates(std::vector<KeyFrame*>{&kf[3], &kf[4]}, true);
        expect("5 queue, first", queued.at(0), {12});
        expect("5 queue, second", queued.at(1), {12});
        if (db.MinScores() != std::vector<float>{0.5f, 1.0f}) { failures++; fprintf(stderr, "kfdb_caller: 5: minScore\n"); }
        const auto lost = db.DetectRelocalizationCandidates(std::vector<Frame*>{&f[3], &f[4]});
        expect("6 frames, first", lost.at(0), {4});
        expect("6 frames, second", lost.at(1), {});
        int32_t size[2];
        int64_t st[8];
        if (drfe_kfdb_size(db.db(), size) != DRFE_OK || drfe_kfdb_stats(db.db(), st) != DRFE_OK) return 2;
        if (size[0] != 7 || size[1] != 5) { failures++; fprintf(stderr, "kfdb_caller: size %d %d\n", size[0], size[1]); }
        db.clear();
        expect("7 after clear", db.DetectLoopCandidates(&kf[5], 0.0f), {});
        if (failures) return 1;
        printf("kfdb_caller ok (%s, %lld loop + %lld relocalisation queries, device calls %lld)\n", mode.c_str(), (long long)st[1],
               (long long)st[3], (long long)st[4]);
    } catch (const std::exception& e) {
        fprintf(stderr, "kfdb_caller: %s\n", e.what());
        return 2;
    }
    return 0;
}
