// The order in which a serial, merging plan plays the recorded branches of a Fork out (model.hip: Op, play) as a host-only rule: which
// recorded launches go out, in which order, and which of them share a launch.  Plain C++17 over the C header's AS_MAX_MULTI: it sees a
// summary of the queues (kinds, waits, five numbers per conv), calls neither HIP nor the library and never looks at a launch's outcome, so
// the whole sequence of steps is made before the first launch -- tests/test_play_order_cpu.py compiles it with g++ and drives it with
// queues built from integers.
//
// THE RULE.  Every queue keeps its own order; a wait holds its queue until every (queue, count) of it has played that many ops.
//   Run ahead.  The queues run in index order, each through its plain launches and through the waits whose dependencies hold.  A `side`
//     launch (a long one on a handful of workgroups) goes to the side stream -- unless no_side -- and PARKS its queue, which ends the
//     queue's run-ahead; a dependency sees a parked queue one op back.  As long as anything ran ahead, the queues run ahead again.
//   Down-sampling steps.  When nothing ran ahead, the unparked heads that are down-sampling steps go out as ONE launch, in queue order, at
//     most AS_MAX_MULTI of them (they are what the towers' next convs wait for) -- before any conv.
//   Conv heads.  Otherwise the conv heads of the unparked queues are the candidates.  None, and a queue is parked: all parked queues are
//     unparked (the calling stream waits for the side stream) and run ahead.  None, nothing parked, ops left: the recorded queues wait for
//     each other, an error.  None and no ops left: the end.
//   Urgent queues.  Unless no_side, a candidate whose queue still has a `side` launch ahead of it is urgent: its convs are what that
//     launch waits for, and every other conv that goes out first is one that could have run beside it.  When some candidates are urgent
//     and some are not, the urgent ones are the candidates.
//   Lone head.  The first candidate that cannot share the tiled kernel's launch (not `mergeable`) goes out alone, so that its queue moves
//     on to heads that can -- except that when it is `direct` (the Cin = 1 kernel's fast form) and at least two candidates are, the
//     direct candidates go out together, at most AS_MAX_MULTI.
//   Row classes.  With every candidate mergeable, the row class (tall: fills the 128-row tile; or not) that holds more work wins, a tie
//     goes to tall; the other class RIDES when tall won and the other's work is <= 0.1 of tall's.  The set is the candidates in queue
//     order whose class is admitted and whose n_prod equals the first pick's, at most AS_MAX_MULTI; a set of one goes out alone.
#pragma once
#include "artspeech_hip.h"
#include <cstddef>
#include <utility>
#include <vector>

namespace play_order {

enum class Kind { Launch, Conv, Wait, Down };      // a plain recorded launch, a conv GEMM, a wait for other queues, a tower down-sampling step

// what the rule sees of a recorded op
struct Op {
    Kind kind = Kind::Launch;
    bool side = false;                             // Launch: a long launch for the side stream
    std::vector<std::pair<int, size_t>> deps;      // Wait: queue `first` has played >= `second` ops
    // Conv, taken once when play begins:
    bool mergeable = false;                        // operand image in, the tiled kernel: it can share a launch
    bool direct = false;                           // the Cin = 1 direct kernel's fast form
    bool tall = false;                             // its rows fill the tall tile (as_fills_tall_tile)
    int n_prod = 0;
    double work = 0;                               // M N (K T + K2)
};
using Queues = std::vector<std::vector<Op>>;

// one thing the executor does; op i of the step is Q[q[i]][at[i]]
struct Step {
    enum What { Launch, Unpark, Down, Conv, Deadlock } what = Launch;
    bool side = false;                             // Launch: on the side stream, and q[0] is parked until the next Unpark
    int n = 0, q[AS_MAX_MULTI] = {};               // Launch: one; Down / Conv: the ops that share the launch, in queue order
    size_t at[AS_MAX_MULTI] = {};
    int candidates = 0;                            // Conv: how many heads the set was chosen from
};

inline std::vector<Step> plan(const Queues& Q, bool no_side)
{
    const int nq = (int)Q.size();
    std::vector<size_t> head(nq, 0);
    std::vector<char> parked(nq, 0);
    std::vector<Step> out;
    std::vector<int> cand, urgent;
    const auto op = [&](int qi) -> const Op& { return Q[qi][head[qi]]; };
    const auto at_head = [&](int qi, Kind k) { return !parked[qi] && head[qi] < Q[qi].size() && op(qi).kind == k; };
    const auto add = [&](Step& st, int qi) { st.q[st.n] = qi; st.at[st.n++] = head[qi]; };
    const auto emit = [&](const Step& st) {        // the step's ops are played
        out.push_back(st);
        for (int i = 0; i < st.n; ++i) ++head[st.q[i]];
    };
    for (;;) {
        bool progress = false;
        for (int qi = 0; qi < nq; ++qi)
            while (head[qi] < Q[qi].size() && !parked[qi]) {
                const Op& o = op(qi);
                if (o.kind == Kind::Wait) {
                    bool ok = true;
                    for (const auto& d : o.deps) ok = ok && head[d.first] - (parked[d.first] ? 1 : 0) >= d.second;
                    if (!ok) break;
                    ++head[qi];
                } else if (o.kind == Kind::Launch) {
                    Step st;
                    st.side = o.side && !no_side;
                    add(st, qi);
                    emit(st);
                    parked[qi] = st.side;
                } else {
                    break;                         // a conv / a down-sampling step: decided below, with the other queues' heads
                }
                progress = true;
            }
        if (progress) continue;
        Step st;
        st.what = Step::Down;
        for (int qi = 0; qi < nq && st.n < AS_MAX_MULTI; ++qi)
            if (at_head(qi, Kind::Down)) add(st, qi);
        if (st.n > 0) { emit(st); continue; }

        st.what = Step::Conv;
        cand.clear();
        bool live = false, any_parked = false;
        for (int qi = 0; qi < nq; ++qi) {
            live = live || head[qi] < Q[qi].size();
            any_parked = any_parked || parked[qi];
            if (at_head(qi, Kind::Conv)) cand.push_back(qi);
        }
        if (cand.empty()) {
            if (any_parked) {
                st.what = Step::Unpark;
                emit(st);
                parked.assign(nq, 0);
                continue;
            }
            if (live) { st.what = Step::Deadlock; emit(st); }
            return out;
        }
        if (!no_side) {
            urgent.clear();
            for (int qi : cand) {
                bool u = false;
                for (size_t k = head[qi]; k < Q[qi].size() && !u; ++k) u = Q[qi][k].side;
                if (u) urgent.push_back(qi);
            }
            if (!urgent.empty() && urgent.size() < cand.size()) cand.swap(urgent);
        }
        st.candidates = (int)cand.size();
        int lone = -1;
        for (size_t i = 0; i < cand.size() && lone < 0; ++i)
            if (!op(cand[i]).mergeable) lone = cand[i];
        if (lone >= 0 && op(lone).direct)
            for (size_t i = 0; i < cand.size() && st.n < AS_MAX_MULTI; ++i)
                if (op(cand[i]).direct) add(st, cand[i]);
        if (lone < 0) {
            double work[2] = {0, 0};
            for (int qi : cand) work[op(qi).tall ? 1 : 0] += op(qi).work;
            const bool tall = work[1] >= work[0], ride = tall && work[0] <= 0.1 * work[1];
            for (size_t i = 0; i < cand.size() && st.n < AS_MAX_MULTI; ++i) {
                const Op& o = op(cand[i]);
                if ((o.tall == tall || ride) && (st.n == 0 || o.n_prod == op(st.q[0]).n_prod)) add(st, cand[i]);
            }
            lone = st.q[0];
        }
        if (st.n < 2) { st.n = 0; add(st, lone); }
        emit(st);
    }
}

}  // namespace play_order
