// Host-only check of csrc/sc_dispatch.hpp's routing (tests/test_dispatch_routing.py builds it with the address and
// undefined-behaviour sanitizers and runs it): every id from -1 to one past the largest model id through both treatments of an
// unlisted id, over the full model list and over the shorter lists the launchers use; the two storage types.
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "../../safe_control_amd/csrc/sc_dispatch.hpp"

static int failures = 0;
static int calls = 0;

static void expect(bool ok, const char* what, int id, int got) {
    if (!ok) { std::printf("FAIL %s: id %d -> %d\n", what, id, got); ++failures; }
}

// the tag a dispatch hands over, and how often it called
static const auto tag_value = [](auto tag) { ++calls; return (int)decltype(tag)::value; };

template <int... IDS>
static void check_list(const char* what) {
    constexpr int ids[] = {IDS...};
    constexpr int last = ids[sizeof...(IDS) - 1];
    for (int id = -1; id <= SC_MODEL_COUNT; ++id) {
        bool listed = false;
        for (int v : ids) listed = listed || v == id;
        calls = 0;
        int got = sc::dispatch_int_last<IDS...>(id, tag_value);
        expect(got == (listed ? id : last) && calls == 1, what, id, got);
        calls = 0;
        got = sc::dispatch_int_or<IDS...>(id, -1000, tag_value);
        expect(got == (listed ? id : -1000) && calls == (listed ? 1 : 0), what, id, got);
    }
}

int main() {
    static_assert(SC_MODEL_COUNT == 8, "a new model id: add it to the full list below");
    check_list<SC_MODEL_DYNAMIC_UNICYCLE2D, SC_MODEL_KINEMATIC_BICYCLE2D, SC_MODEL_KINEMATIC_BICYCLE2D_C3BF,
               SC_MODEL_KINEMATIC_BICYCLE2D_DPCBF, SC_MODEL_SINGLE_INTEGRATOR2D, SC_MODEL_DOUBLE_INTEGRATOR2D, SC_MODEL_QUAD2D,
               SC_MODEL_UNICYCLE2D>("all models");
    // the rollout's order: the list is not sorted, and the entry that serves the unlisted ids is not the largest
    check_list<SC_MODEL_DYNAMIC_UNICYCLE2D, SC_MODEL_KINEMATIC_BICYCLE2D, SC_MODEL_UNICYCLE2D, SC_MODEL_KINEMATIC_BICYCLE2D_C3BF,
               SC_MODEL_SINGLE_INTEGRATOR2D, SC_MODEL_DOUBLE_INTEGRATOR2D, SC_MODEL_KINEMATIC_BICYCLE2D_DPCBF>("rollout models");
    check_list<SC_MODEL_SINGLE_INTEGRATOR2D, SC_MODEL_DOUBLE_INTEGRATOR2D, SC_MODEL_DYNAMIC_UNICYCLE2D>("sensing models");
    check_list<SC_MODEL_KINEMATIC_BICYCLE2D, SC_MODEL_QUAD2D>("two models");
    check_list<SC_MODEL_QUAD2D>("one model");

    for (int io : {SC_DTYPE_F32, SC_DTYPE_F64, -1, 2}) {                  // whatever is not f32 is stored as f64, as the ladders had it
        calls = 0;
        const int bytes = sc::dispatch_io(io, [](auto tio) {
            using T = sc::tag_t<decltype(tio)>;
            static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "storage is f32 or f64");
            ++calls;
            return (int)sizeof(T);
        });
        expect(bytes == (io == SC_DTYPE_F32 ? 4 : 8) && calls == 1, "storage type", io, bytes);
    }
    // nested, as a launcher uses them: the inner callable sees both tags
    const int both = sc::dispatch_io(SC_DTYPE_F32, [](auto tio) {
        return sc::dispatch_int_last<3, 5>(5, [&](auto id) { return (int)sizeof(sc::tag_t<decltype(tio)>) * 100 + decltype(id)::value; });
    });
    expect(both == 405, "nested", 5, both);

    if (failures) return 1;
    std::printf("dispatch routing ok\n");
    return 0;
}
