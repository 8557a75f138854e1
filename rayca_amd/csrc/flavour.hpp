// flavour.hpp -- which traversal a kernel is instantiated for, and how the host turns run-time choices into template arguments.
// Host code of both units that hold traversal kernels (kernels.hip through select.inc, refill.hip): the one list of flavours.
#pragma once
#include <type_traits>

namespace rayca {

// Traversal flavours that are actually instantiated (the full cross product would be 32 per kernel):
//   kTravFast        ordered, conservative slabs, binary tree, stack entirely in LDS   <- production, generation 0
//   kTravFastSpill   same with the global spill path (trees whose stack need exceeds the LDS part)
//   kTravFastWide    ordered, conservative slabs, 4-wide tree, spill                   <- production, bounce generations
//   kTravExact       ordered, the reference's slab arithmetic, binary, spill           <- RAYCA_BUILDER_REFERENCE
//   kTravExactAll    exhaustive, exact slabs, binary, spill                             <- visits the reference's leaves
//   kTravFastAll     exhaustive, conservative slabs, binary, spill                      <- verification of the SAH tree
//   kTrav*Half       the three production flavours on the fp16 node arrays (DevNodeH / DevNode4H)
enum Trav { kTravFast, kTravFastSpill, kTravFastWide, kTravExact, kTravExactAll, kTravFastAll, kTravFastHalf, kTravFastSpillHalf, kTravFastWideHalf, kTravCount };

// The kernel, the stack plan (plan_stack, bind_stack) and the root the kernel starts from all follow these bits: whoever needs
// "has a spill path" or "walks the 4-wide tree" of a launch asks the traits of the Trav it launches.
struct TravTraits {
  bool ordered, fast, wide, spill, half;
};
constexpr TravTraits kTravTraits[kTravCount] = {
    // ORDERED FAST  WIDE   SPILL  HALF
    {true,  true,  false, false, false},   // kTravFast
    {true,  true,  false, true,  false},   // kTravFastSpill
    {true,  true,  true,  true,  false},   // kTravFastWide
    {true,  false, false, true,  false},   // kTravExact
    {false, false, false, true,  false},   // kTravExactAll
    {false, true,  false, true,  false},   // kTravFastAll
    {true,  true,  false, false, true},    // kTravFastHalf
    {true,  true,  false, true,  true},    // kTravFastSpillHalf
    {true,  true,  true,  true,  true},    // kTravFastWideHalf
};
constexpr const TravTraits& traits(Trav t) { return kTravTraits[t]; }

// a flavour as a type: what a kernel picker names its template arguments with
template <Trav T>
struct TravTag {
  static constexpr Trav trav = T;
  static constexpr bool ORDERED = kTravTraits[T].ordered, FAST = kTravTraits[T].fast, WIDE = kTravTraits[T].wide, SPILL = kTravTraits[T].spill,
                        HALF = kTravTraits[T].half;
};

// f(TravTag<t>{}): the only place that lists the flavours
template <typename F>
auto with_trav(Trav t, F&& f) {
  switch (t) {
    case kTravFast:          return f(TravTag<kTravFast>{});
    case kTravFastSpill:     return f(TravTag<kTravFastSpill>{});
    case kTravFastWide:      return f(TravTag<kTravFastWide>{});
    case kTravExact:         return f(TravTag<kTravExact>{});
    case kTravExactAll:      return f(TravTag<kTravExactAll>{});
    case kTravFastHalf:      return f(TravTag<kTravFastHalf>{});
    case kTravFastSpillHalf: return f(TravTag<kTravFastSpillHalf>{});
    case kTravFastWideHalf:  return f(TravTag<kTravFastWideHalf>{});
    default:                 return f(TravTag<kTravFastAll>{});
  }
}

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): run-time flags as template arguments.  Every combination of the
// flags instantiates f, so a picker names exactly the kernels that its body can spell.
template <typename F>
auto with_flags(F&& f) {
  return f();
}
template <typename F, typename... Rest>
auto with_flags(F&& f, bool b, Rest... rest) {
  auto bound = [&](auto c) { return with_flags([&](auto... cs) { return f(c, cs...); }, rest...); };
  return b ? bound(std::true_type{}) : bound(std::false_type{});
}
// the two composed: f(TravTag<t>{}, std::bool_constant<b>{}...)
template <typename F, typename... Flags>
auto with_flavour(F&& f, Trav t, Flags... flags) {
  return with_trav(t, [&](auto tag) { return with_flags([&](auto... cs) { return f(tag, cs...); }, flags...); });
}

}  // namespace rayca
