// Probe of artspeech_amd/csrc/play_order.h for tests/test_play_order_cpu.py: recorded queues built from integers, one "case step" line per
// step of the play-out.  A step reads L<q>.<i> (plain launch of op i of queue q), S<q>.<i> (the same on the side stream: q is parked),
// U (unpark all), D<q>.<i>+... (one down-sampling launch), G<q>.<i>+... (one conv launch), E (the queues wait for each other); `end`
// closes a play-out that ended without an error.
#include "play_order.h"
#include <cstdio>
#include <string>

using namespace play_order;

static Op launch(bool side = false) { Op o; o.kind = Kind::Launch; o.side = side; return o; }
static Op down() { Op o; o.kind = Kind::Down; return o; }
static Op wait(std::vector<std::pair<int, size_t>> deps) { Op o; o.kind = Kind::Wait; o.deps = deps; return o; }
// a conv that can share the tiled kernel's launch, of `work`, tall or short rows
static Op conv(double work, bool tall, int n_prod = 3)
{
    Op o;
    o.kind = Kind::Conv; o.mergeable = true; o.tall = tall; o.work = work; o.n_prod = n_prod;
    return o;
}
static Op unmergeable(bool direct) { Op o = conv(100, true); o.mergeable = false; o.direct = direct; return o; }
static const bool TALL = true, SHORT = false;

static void play(const char* name, const Queues& Q, bool no_side = false)
{
    bool failed = false;
    for (const Step& st : plan(Q, no_side)) {
        std::string s = st.what == Step::Launch ? (st.side ? "S" : "L") : st.what == Step::Unpark ? "U" : st.what == Step::Down ? "D"
                        : st.what == Step::Conv ? "G" : "E";
        for (int i = 0; i < st.n; ++i) s += (i ? "+" : "") + std::to_string(st.q[i]) + "." + std::to_string(st.at[i]);
        printf("%s %s\n", name, s.c_str());
        failed = failed || st.what == Step::Deadlock;
    }
    if (!failed) printf("%s end\n", name);
}
// queues of one op each: the heads of one decision
static Queues heads(std::vector<Op> ops)
{
    Queues Q;
    for (const Op& o : ops) Q.push_back({o});
    return Q;
}

int main()
{
    // 1. fork / join: queue 0 is the calling stream (it only joins), A = queue 1, B = queue 2
    play("fork_join", {{wait({{1, 4}, {2, 3}})},
                       {wait({{0, 0}}), launch(), conv(100, TALL), launch()},
                       {wait({{0, 0}}), conv(100, TALL), conv(100, TALL)}});

    // 2. row classes
    play("rows_short_holds_more", heads({conv(100, TALL), conv(50, TALL), conv(200, SHORT)}));
    play("rows_ride_at_a_tenth", heads({conv(1000, TALL), conv(100, SHORT)}));
    play("rows_no_ride_above_a_tenth", heads({conv(1000, TALL), conv(101, SHORT)}));
    play("rows_tie_goes_to_tall", heads({conv(100, SHORT), conv(100, TALL)}));

    // 3. n_prod
    play("n_prod_3_1_3", heads({conv(100, TALL, 3), conv(100, TALL, 1), conv(100, TALL, 3)}));

    // 4. heads that cannot share the tiled kernel's launch
    play("lone_goes_first", heads({conv(100, TALL), unmergeable(false)}));
    play("direct_pair_together", heads({conv(100, TALL), unmergeable(true), unmergeable(true)}));
    play("direct_single", heads({unmergeable(true)}));
    play("direct_single_beside_mergeable", heads({conv(100, TALL), unmergeable(true)}));
    play("lone_not_direct_before_a_direct", heads({conv(100, TALL), unmergeable(false), unmergeable(true)}));

    // 5. AS_MAX_MULTI (6)
    play("seven_convs", heads(std::vector<Op>(7, conv(100, TALL))));
    {
        std::vector<Op> h(7, down());
        h.push_back(conv(100, TALL));
        play("seven_downs_and_a_conv", heads(h));
    }
    play("conv_between_downs", heads({down(), conv(100, TALL), down()}));

    // 6. a side launch: queue 0 joins, D = queue 1 (conv, the long launch r, a launch p), E = queue 2 (two convs), F = queue 3 (after r)
    const Queues side = {{wait({{1, 4}, {2, 3}, {3, 2}})},
                         {wait({{0, 0}}), conv(100, TALL), launch(true), launch()},
                         {wait({{0, 0}}), conv(100, TALL), conv(100, TALL)},
                         {wait({{1, 3}}), launch()}};
    play("side", side);
    play("side_no_side", side, true);
    play("side_every_head_urgent", {{conv(100, TALL), launch(true)}, {conv(100, TALL), launch(true)}});

    // 7. two queues that wait for each other's launch
    play("deadlock", {{wait({{1, 2}}), launch()}, {wait({{0, 2}}), launch()}});
    return 0;
}
