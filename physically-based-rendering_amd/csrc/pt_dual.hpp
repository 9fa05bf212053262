// The lane state machine with TWO paths per lane ("phased-dual", plan 6) — included by pt_kernel.hpp inside namespace ptk.
//
// pathTracingPhased hides the latency of a walk's dependent fetches behind six waves per SIMD; this kernel hides it behind
// the lane's OTHER path: every lane carries two path slots A and B (128 paths per wave at 4 waves per SIMD), and the node
// phase of the two walks is software-pipelined — A's next records are requested, then B's records are waited for and tested
// while A's are in flight, and the other way round.  Built in round 4 and measured against the six
// other plans, all bit-identical: 1.02 - 1.03x of phased-mid on the Sponza-class scene (2099 - 2102 against 2048 - 2053 Msamples/s at
// 1080p in 32-frame launches, same box), 0.97x on the Dragon-class scene, 0.89x on the hairball — the tuner takes it where it
// wins (profiles/r04/experiments/two_paths_per_lane.txt).
//
//   node phase   nodePhaseDualPipe (below)
//   leaf phase   POOLED: a lane tests the leaf of whichever of its slots stands on one (A first; the other in the next
//                round) — one pass of the face tests serves lanes of both slots
//   shade phase  POOLED the same way: a lane shades whichever slot waits for shading; the threshold counts lanes
// In registers per slot: ray, 1 / direction, cursor, closest hit, the parked leaf, mode, the walk's counters (17).  Everything
// else a path carries between bounces (PixelState's cold half: 16 dwords) lives in LDS, in four lane-linear 16-byte planes
// per slot behind the staged tree top (P.slotBase; 2 x 64 B x 1024 lanes = 128 KiB, which leaves 1016 staged records), and is
// in registers only while its slot is shaded.  121 VGPRs (125 up to round 14), no scratch (BRDF 1 without lights).
// Per path the sequence of visits, face tests and random draws is the reference's (pathtracing.cl:207-334, pt_bvh.cl:75-125):
// same image, same debug image, same counters.
#ifdef PT_NODE_PHASE_ASM

// ---- the node phase of two walks, software-pipelined -------------------------------------------------------------------
// Walk A's records live in v[46:53], walk B's in v[64:71], the slab test's temporaries in v54 - v63 (as nodePhaseAsm), the
// cursors in v53 / v71, the records' last words (round 11; as nodePhaseAsm since round 3).  s[86:87] / s[88:89] = the lanes whose
// walk A / B goes on, VCC != 0 = "the last fetch — the OTHER walk's, seen from a wait — issued loads of both kinds".
// A wait in front of a slab test is COUNTED — s_waitcnt vmcnt(2) lgkmcnt(2): everything but the other walk's two loads of
// each kind, which were issued later — only when that other fetch did issue both kinds (an instruction with an empty EXEC
// may or may not count); otherwise everything is waited for.  A walk's next records are requested as soon as its visit has
// decided which lanes go on — the exit test runs under the requests; when `keep` or fewer walks go on, each walk takes the visit
// its request is for (a node phase may always run one visit longer) and the phase ends with nothing in flight.
// Round 12 (request first): the cold request leaves three scalar-unit steps behind the cursor's v_cndmask — the walk's mask
// less the lanes that just parked, one signed compare against numHotBytes (false for an ended walk's negative cursor: no alive
// test), s_and_saveexec —; the resident lanes (one unsigned compare, which is the alive test too), the walk's next mask, the
// flag and "nobody goes on" (no branch any more: an empty request, then the empty-walk skip) stand behind the global loads, and
// walk A's last visit takes the counted wait.  The invariants are written out at PT_DUAL_VISIT_AND_FETCH.
// Per walk-visit 24 vector instructions (nodePhaseAsm: 22; one of the 24 is the v_cmpx that finds the resident lanes, which
// replaced the alive compare) and 11 scalar ones, the wait among them (nodePhaseAsm: 8), plus the
// loop's five per pair of visits (two s_bcnt1: a lane may hold two walks, so no combined mask counts them).  Up to round 10: 24
// and 14 — round 11 took the cursor's copy and the parked lanes' tNear select out of the chain between a record's arrival and
// the next request (the copy is gone, tNear and the leaf word are kept behind the request, under EXEC = the parked lanes, which
// replaces the parked masks and their collection when the phase ends), carries the flag in VCC (one s_cselect_b64 and one
// s_cbranch_vccz instead of two s_cselect_b32, s_cmp and a branch) and lets s_and_saveexec write the walk's mask itself.
// Registers v72 / v73, s80 - s82 and s[90:93] fell idle by that.  What the loop's shape is worth, measured
// step by step on the Sponza-class scene (profiles/r04/experiments/two_paths_per_lane.txt, 7.): the uncommon cases (a full
// wait, a walk without lanes) out of line, ONE taken branch per iteration instead of three: +1.1 %; everything that does not
// need the records (EXEC, the visit counter) in front of the wait instead of behind it: +0.9 %; the next request issued
// straight from the two masks, its bookkeeping behind the loads, and the parked lanes' leaf words collected once, when the
// phase ends: +0.3 %.  The loop is bound by the length of its dependent chain, not by instruction issue.
#define PT_DUAL_SLAB( n0a, n0b, n0c, n0d, n1a, n1b, oxy, ozi, ixy ) \
		"v_pk_add_f32 v[54:55], v[" n0a ":" n0b "], " oxy " neg_lo:[0,1] neg_hi:[0,1]\n" \
		"v_pk_add_f32 v[56:57], v[" n0c ":" n0d "], " oxy " neg_lo:[0,1] neg_hi:[0,1]\n" \
		"v_pk_add_f32 v[58:59], v[" n1a ":" n1b "], " ozi " op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n" \
		"v_pk_mul_f32 v[54:55], " ixy ", v[54:55]\n" \
		"v_pk_mul_f32 v[56:57], " ixy ", v[56:57]\n" \
		"v_pk_mul_f32 v[58:59], " ozi ", v[58:59] op_sel:[1,0]\n" \
		"v_min_f32 v60, v54, v56\n" \
		"v_min_f32 v61, v55, v57\n" \
		"v_min_f32 v62, v58, v59\n" \
		"v_max3_f32 v60, v60, v61, v62\n" \
		"v_max_f32 v61, v54, v56\n" \
		"v_max_f32 v63, v58, v59\n" \
		"v_max_f32 v62, v55, v57\n" \
		"v_min3_f32 v61, v61, v62, v63\n"
// A walk's request: the cold records first — the global load is what the visit waits for —, then the resident ones (round 11).
// VCC carries the flag "this fetch issued loads of both kinds" to the other walk's wait: the compare leaves the cold lanes
// in VCC (a compare writes 0 for the lanes outside EXEC), s_and_saveexec makes them EXEC, s_xor the resident ones with
// SCC = "there are some", and s_cselect_b64 keeps VCC where SCC is set and clears it otherwise — VCC != 0 exactly when both
// sets have lanes.  Nothing between here and the other walk's wait writes VCC (a visit's compares write s[94:95] / s[98:99]).
#define PT_DUAL_FETCH( walk, cur, n0, n1lo, n1hi, skip ) \
		"s_mov_b64 exec, " walk "\n" \
		"s_cbranch_execz " skip "9f\n" \
		"v_cmp_le_i32 vcc, %[numHotBytes], " cur "\n" \
		"s_and_saveexec_b64 s[94:95], vcc\n" \
		"global_load_dwordx4 v[" n0 "], " cur ", %[nodes]\n" \
		"global_load_dwordx4 v[" n1lo ":" n1hi "], " cur ", %[nodes] offset:16\n" \
		"s_xor_b64 exec, exec, s[94:95]\n" \
		"s_cselect_b64 vcc, vcc, 0\n" \
		"ds_read_b128 v[" n0 "], " cur "\n" \
		"ds_read_b128 v[" n1lo ":" n1hi "], " cur " offset:16\n" \
	skip ":\n"
// the counted wait; the uncommon case (the other fetch did not issue both kinds) waits for everything, out of line
#define PT_DUAL_WAIT( full, go ) \
		"s_cbranch_vccz " full "f\n" \
		"s_waitcnt vmcnt(2) lgkmcnt(2)\n" \
	go ":\n"
// a walk without lanes requests nothing: its flag says so (out of line)
#define PT_DUAL_FETCH_NONE( skip ) \
	skip "9:\n" \
		"s_mov_b64 vcc, 0\n" \
		"s_branch " skip "b\n"
#define PT_DUAL_WAIT_FULL( full, go ) \
	full ":\n" \
		"s_waitcnt vmcnt(0) lgkmcnt(0)\n" \
		"s_branch " go "b\n"
// One walk's visit: what does not need the records stands in front of the wait; behind it the slab test, the hit chain, and
// s[98:99] = the lanes that stand on a hit leaf.  The cursor lives in the record's last register (v53 / v71), as in nodePhaseAsm:
// the last word IS the reference to continue at unless the box is a hit container, a load may overwrite its own address
// register, and a lane that has left the walk — parked, ended, or sitting the phase out — is in no later fetch of that walk,
// so its last word stays where it is until the phase ends (the same holds for a parked lane's leaf word in v52 / v70).
// W = "A" / "B"; walk = the walk's mask pair; r0..r7 = the eight record registers.
#define PT_DUAL_VISIT_CORE( ... ) PT_DUAL_VISIT_CORE_( __VA_ARGS__ )      /* (the register lists are macros: expanded before the call) */
#define PT_DUAL_VISIT_CORE_( skip, wait, W, walk, r0, r1, r2, r3, r4, r5, r6, r7 ) \
		"s_mov_b64 exec, " walk "\n" \
		"s_cbranch_execz " skip "f\n" \
		"v_add_u32 %[visits" W "], 1, %[visits" W "]\n" \
		wait \
		PT_DUAL_SLAB( r0, r1, r2, r3, r4, r5, "%[oxy" W "]", "%[ozi" W "]", "%[ixy" W "]" ) \
		"v_cmpx_lt_f32 %[eps], v61\n" \
		"v_cmpx_gt_f32 %[rayT" W "], v60\n" \
		"v_cmpx_le_f32 v60, v61\n" \
		"v_cmp_gt_i32 s[98:99], 0, v" r6 "\n" \
		"v_cndmask_b32 v" r7 ", v" r6 ", v" r7 ", s[98:99]\n"
// what a visit owes the lanes that parked on a hit leaf: the leaf's word and tNear (a slab temporary the other walk's visit
// overwrites) — behind the request, which does not need them
#define PT_DUAL_KEEP_PARKED( W, r6 ) \
		"s_mov_b64 exec, s[98:99]\n" \
		"v_mov_b32 %[tNear" W "], v60\n" \
		"v_mov_b32 %[leafWord" W "], v" r6 "\n"
// ... and, in the loop, the request for its next records at once (round 12: request first).  Behind the v_cndmask that puts
// the next reference into the cursor there are three scalar-unit steps up to the first global load (up to round 11: six) —
//     s_andn2 exec, walk, s[98:99]          the walk's lanes that did not just park
//     v_cmp_le_i32 vcc, numHotBytes, cursor the cold ones among them: numHotBytes >= 0, so the SIGNED compare is false for
//                                           every lane whose walk has ended (cursor < 0) — no alive test in front of it
//     s_and_saveexec s[94:95], vcc          EXEC = the cold lanes
// — and behind the two loads the resident lanes (numHotBytes >u cursor, UNSIGNED: true exactly for 0 <= cursor <
// numHotBytes, so it is the alive test as well; v_cmpx writes EXEC and s[94:95] alike), their two LDS reads, the walk's next
// mask = cold | resident, and the flag.  Eight instructions around the four memory ones, as before.  Invariants:
//  - A cold lane's cursor register is overwritten when its load returns, at any time after issue.  Every instruction behind
//    the request that reads the cursor therefore runs with the cold lanes out of EXEC: the resident set is derived under
//    EXEC = ( walk & ~parked ) & ~cold (s_xor: cold is a subset), never under the walk's whole mask.
//  - A lane is in at most one of { cold, resident, parked, ended }.  A parked or ended lane is in no later fetch of that walk,
//    so its last word, leaf word and tNear stay where they are until the phase ends (PT_DUAL_KEEP_PARKED reads them behind
//    the request, under EXEC = s[98:99]).
//  - numHotBytes = 0 (knob lds_slots = 0): no resident lane ever, the global loads carry every lane that goes on.
//    numHotBytes at or above the tree's size: no cold lane ever, the global loads issue with an empty EXEC.
//  - The flag: VCC = the cold lanes, kept by s_cselect_b64 only where s_cmp_lg_u64 found resident lanes too — VCC != 0
//    exactly when both sets have lanes; a fetch with an empty cold set, an empty resident set, or both leaves VCC = 0, and
//    the other walk's wait is then for everything (whether an instruction with an empty EXEC counts is not known here).
//    Nothing between here and the other walk's wait writes VCC.
//  - "Nobody goes on" does not branch at all any more: that request has neither kind of lane (four memory instructions with
//    EXEC = 0, which write no register), it leaves VCC = 0 and the walk's mask = 0, and the walk's next visit is the one
//    PT_DUAL_VISIT_CORE has always skipped for a walk without lanes (s_cbranch_execz, out of line: VCC = 0) — no visit runs
//    on records nobody asked for.
#define PT_DUAL_VISIT_AND_FETCH( ... ) PT_DUAL_VISIT_AND_FETCH_( __VA_ARGS__ )
#define PT_DUAL_VISIT_AND_FETCH_( skip, empty, wait, W, walk, r0, r1, r2, r3, r4, r5, r6, r7 ) \
		PT_DUAL_VISIT_CORE( empty, wait, W, walk, r0, r1, r2, r3, r4, r5, r6, r7 ) \
		"s_andn2_b64 exec, " walk ", s[98:99]\n" \
		"v_cmp_le_i32 vcc, %[numHotBytes], v" r7 "\n" \
		"s_and_saveexec_b64 s[94:95], vcc\n" \
		"global_load_dwordx4 v[" r0 ":" r3 "], v" r7 ", %[nodes]\n" \
		"global_load_dwordx4 v[" r4 ":" r7 "], v" r7 ", %[nodes] offset:16\n" \
		"s_xor_b64 exec, exec, s[94:95]\n" \
		"v_cmpx_gt_u32_e64 s[94:95], %[numHotBytes], v" r7 "\n" \
		"ds_read_b128 v[" r0 ":" r3 "], v" r7 "\n" \
		"ds_read_b128 v[" r4 ":" r7 "], v" r7 " offset:16\n" \
		"s_or_b64 " walk ", vcc, s[94:95]\n" \
		"s_cmp_lg_u64 s[94:95], 0\n" \
		"s_cselect_b64 vcc, vcc, 0\n" \
		PT_DUAL_KEEP_PARKED( W, r6 ) \
	skip ":\n"
// a walk that has no lanes left takes no visit and issues nothing — which the other walk's wait must know: VCC would still
// hold that other walk's own flag (out of line)
#define PT_DUAL_VISIT_EMPTY( empty, skip ) \
	empty ":\n" \
		"s_mov_b64 vcc, 0\n" \
		"s_branch " skip "b\n"
// The visits the phase ends with (no request follows).  Walk A's takes the counted wait like every visit of the loop (round
// 12): when the loop is left VCC is still the flag of walk B's last fetch — between PT_DUAL_VISIT_AND_FETCH( B ) and here stand
// s_cselect_b64 (which wrote it), PT_DUAL_KEEP_PARKED (s_mov exec, two v_mov), s_bcnt1 x 2, s_add, s_cmp and the branch
// that fell through, which write EXEC and SCC only; a walk B without lanes set VCC = 0 (PT_DUAL_VISIT_EMPTY) — and B's loads
// are the two youngest of each kind, so A's slab test runs while B's records are still on their way.  Walk B's waits for
// everything: nothing was issued after its request (and A's visit has written VCC by then: its v_cmpx do).
#define PT_DUAL_VISIT_LAST( ... ) PT_DUAL_VISIT_LAST_( __VA_ARGS__ )
#define PT_DUAL_VISIT_LAST_( skip, wait, W, walk, r0, r1, r2, r3, r4, r5, r6, r7 ) \
		PT_DUAL_VISIT_CORE( skip, wait, W, walk, r0, r1, r2, r3, r4, r5, r6, r7 ) \
		PT_DUAL_KEEP_PARKED( W, r6 ) \
	skip ":\n"
#define PT_DUAL_REGS_A "46", "47", "48", "49", "50", "51", "52", "53"
#define PT_DUAL_REGS_B "64", "65", "66", "67", "68", "69", "70", "71"

// walkA / walkB: the lanes whose slot A / B walks (wave masks: the caller's ballots of mode == MODE_NODE, which implies a cursor
// >= 0); refA / refB: the slots' cursors, handed over as they are — a lane outside its walk's mask is in no fetch and no visit of
// that walk, so its cursor, leaf word and tNear come back untouched.  A lane whose walk parks on a hit leaf gets the leaf's word
// and tNear in leafWordA / tNearA (leafWordB / tNearB): the caller hands the slots' own fields over (0 for every walking lane:
// the leaf phase and startWalkDual clear the word) and reads != 0 as "parked"; tNear is defined only where the word is != 0.
// nodes: P.nodes as the caller holds it — an opaque scalar, see pathTracingDual.
// The z operands are ONE pair per walk, { origin.z, 1 / dir.z } (round 15): the slab test picks the half it needs by op_sel
// (v_pk_add: the low half for both results; v_pk_mul: the high half for both), where it used to read { z, z } pairs that the
// caller rebuilt with a v_mov each, four per round.
PT_DEV void nodePhaseDualPipe(
	const DevParams& P, const float4* nodes,
	const f2v oxyA, const f2v oziA, const f2v ixyA, float rayTA,
	const f2v oxyB, const f2v oziB, const f2v ixyB, float rayTB,
	int keep, unsigned long long walkA, unsigned long long walkB, int& refA, int& refB, unsigned& visitsA, unsigned& visitsB,
	int& leafWordA, float& tNearA, int& leafWordB, float& tNearB
) {
	const float eps = EPSILON5;
	keep = __builtin_amdgcn_readfirstlane( keep );

	asm volatile(
		"s_waitcnt lgkmcnt(0)\n"
		"s_mov_b64 s[84:85], exec\n"
		"s_mov_b64 s[86:87], %[walkA]\n"
		"s_mov_b64 s[88:89], %[walkB]\n"
		"v_mov_b32 v53, %[refA]\n"
		"v_mov_b32 v71, %[refB]\n"
		PT_DUAL_FETCH( "s[86:87]", "v53", "46:49", "50", "53", "10" )
		PT_DUAL_FETCH( "s[88:89]", "v71", "64:67", "68", "71", "11" )
	"1:\n"
		// walk A on its records (B's request, issued after them, may stay in flight), and A's next request; then B the same way
		PT_DUAL_VISIT_AND_FETCH( "4", "22", PT_DUAL_WAIT( "12", "13" ), "A", "s[86:87]", PT_DUAL_REGS_A )
		PT_DUAL_VISIT_AND_FETCH( "5", "23", PT_DUAL_WAIT( "15", "16" ), "B", "s[88:89]", PT_DUAL_REGS_B )
		"s_bcnt1_i32_b64 s96, s[86:87]\n"
		"s_bcnt1_i32_b64 s97, s[88:89]\n"
		"s_add_i32 s96, s96, s97\n"
		"s_cmp_gt_i32 s96, %[keep]\n"
		"s_cbranch_scc1 1b\n"
		// enough walks have left.  The records that are on their way are not dropped: each walk takes that visit (a node phase
		// may always run one visit longer), and the phase ends with nothing in flight
		PT_DUAL_VISIT_LAST( "6", PT_DUAL_WAIT( "24", "25" ), "A", "s[86:87]", PT_DUAL_REGS_A )
		PT_DUAL_VISIT_LAST( "7", "s_waitcnt vmcnt(0) lgkmcnt(0)\n", "B", "s[88:89]", PT_DUAL_REGS_B )
		"s_waitcnt vmcnt(0) lgkmcnt(0)\n"
		"s_mov_b64 exec, s[84:85]\n"
		"v_mov_b32 %[refA], v53\n"
		"v_mov_b32 %[refB], v71\n"
		"s_branch 21f\n"
		PT_DUAL_WAIT_FULL( "12", "13" )
		PT_DUAL_WAIT_FULL( "15", "16" )
		PT_DUAL_WAIT_FULL( "24", "25" )
		PT_DUAL_FETCH_NONE( "10" )
		PT_DUAL_FETCH_NONE( "11" )
		PT_DUAL_VISIT_EMPTY( "22", "4" )
		PT_DUAL_VISIT_EMPTY( "23", "5" )
	"21:\n"
		: [refA] "+v"( refA ), [refB] "+v"( refB ), [visitsA] "+v"( visitsA ), [visitsB] "+v"( visitsB ),
		  [leafWordA] "+v"( leafWordA ), [tNearA] "+v"( tNearA ), [leafWordB] "+v"( leafWordB ), [tNearB] "+v"( tNearB )
		: [oxyA] "v"( oxyA ), [oziA] "v"( oziA ), [ixyA] "v"( ixyA ), [rayTA] "v"( rayTA ),
		  [oxyB] "v"( oxyB ), [oziB] "v"( oziB ), [ixyB] "v"( ixyB ), [rayTB] "v"( rayTB ),
		  [keep] "s"( keep ), [walkA] "s"( walkA ), [walkB] "s"( walkB ), [numHotBytes] "s"( P.numHotBytes ), [nodes] "s"( nodes ), [eps] "s"( eps )
		: "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63",
		  "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71",
		  // (v72 / v73 — the cursors until round 11 — and s80 - s82, s[90:93] — the flags and the parked masks — are not used any
		  // more and stay reserved: with them free hipcc allocates the kernels' registers differently — 123 vector registers
		  // instead of 125, the same four waves —, and pathTracingDual<0, false, true> then keeps 20 B in scratch, which it did not)
		  "v72", "v73",
		  "s80", "s81", "s82", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "s96", "s97", "s98", "s99", "vcc", "scc"
	);
}
#undef PT_DUAL_FETCH
#undef PT_DUAL_WAIT
#undef PT_DUAL_WAIT_FULL
#undef PT_DUAL_FETCH_NONE
#undef PT_DUAL_VISIT_CORE
#undef PT_DUAL_VISIT_CORE_
#undef PT_DUAL_VISIT_AND_FETCH
#undef PT_DUAL_VISIT_AND_FETCH_
#undef PT_DUAL_VISIT_LAST_
#undef PT_DUAL_VISIT_EMPTY
#undef PT_DUAL_KEEP_PARKED
#undef PT_DUAL_VISIT_LAST
#undef PT_DUAL_REGS_A
#undef PT_DUAL_REGS_B
#undef PT_DUAL_SLAB

// ---- a path slot: what a path keeps in registers while it is not being shaded ----------------------------------------
struct DualSlot {
	Ray ray;
	f3 invDir;
	int cur;            // cursor (byte offset of the next record); < 0: the walk has ended
	float t;            // closest hit so far
	int face;
	int leafWord;       // != 0: parked on this hit leaf (MODE_LEAF)
	float leafTNear;
	int mode;
	unsigned nodes, tris;   // of the current walk(s) since the slot was last shaded: added to the path's counters there
};

// the cold half of a path's state: four lane-linear 16-byte planes per slot in LDS, behind the staged tree top
PT_DEV float4* coldPlane( const DevParams& P, int slot, int plane ) {
	return (float4*) ( (char*) gHotNodes + P.slotBase ) + ( slot * 4 + plane ) * PBR_BLOCK + (int) threadIdx.x;
}

PT_DEV void loadCold( const DevParams& P, int slot, PixelState& st ) {
	const float4 a = *coldPlane( P, slot, 0 ), b = *coldPlane( P, slot, 1 ), c = *coldPlane( P, slot, 2 ), d = *coldPlane( P, slot, 3 );
	st.slot = __float_as_uint( a.x ); st.frame = __float_as_int( a.y ); st.sample = __float_as_int( a.z ); st.finalColor.x = a.w;
	st.finalColor.y = b.x; st.finalColor.z = b.y; st.secondaryPaths = __float_as_uint( b.z ); st.focus = b.w;
	st.seed = c.x; st.dbgNodes = __float_as_uint( c.y ); st.dbgTris = __float_as_uint( c.z ); st.color.x = c.w;
	st.color.y = d.x; st.color.z = d.y; st.depth = __float_as_int( d.z ); st.depthAdded = __float_as_int( d.w );
}

PT_DEV void storeCold( const DevParams& P, int slot, const PixelState& st ) {
	*coldPlane( P, slot, 0 ) = make_float4( __uint_as_float( st.slot ), __int_as_float( st.frame ), __int_as_float( st.sample ), st.finalColor.x );
	*coldPlane( P, slot, 1 ) = make_float4( st.finalColor.y, st.finalColor.z, __uint_as_float( st.secondaryPaths ), st.focus );
	*coldPlane( P, slot, 2 ) = make_float4( st.seed, __uint_as_float( st.dbgNodes ), __uint_as_float( st.dbgTris ), st.color.x );
	*coldPlane( P, slot, 3 ) = make_float4( st.color.y, st.color.z, __int_as_float( st.depth ), __int_as_float( st.depthAdded ) );
}

template<bool LIGHTS>
PT_DEV void startWalkDual( const DevParams& P, DualSlot& s ) {
	s.invDir = mk3( div1( 1.0f, s.ray.dir.x ), div1( 1.0f, s.ray.dir.y ), div1( 1.0f, s.ray.dir.z ) );
	s.cur = firstNode( P, s.ray.dir ).ref;
	Hit h;
	h.t = inff();
	h.face = 0;

	if( LIGHTS ) {
		traverseLights( P, s.ray, h );
	}

	s.t = h.t;
	s.face = h.face;
	s.leafWord = 0;
	s.leafTNear = 0.0f;
	s.mode = MODE_NODE;
}

// P.phPark: a node phase ends once that many of the wave's WALKS (of up to 128) have left it; P.phShade: a shade phase
// runs once that many LANES have a slot waiting (or nothing else is left to do).  Measured best: 28 / 48.
template<int BRDF, bool SHADOW, bool LIGHTS>
__global__ __launch_bounds__( PBR_BLOCK, 4 ) void pathTracingDual( const DevParams P ) {
	const float4* lds = gHotNodes;
	stageHotNodes( P, gHotNodes );
	LaneCounters cnt;
	cnt.nodes = cnt.tris = cnt.hits = cnt.paths = 0;
	DualSlot A, B;
	A.mode = B.mode = MODE_DONE;
	A.cur = B.cur = -1;
	A.leafWord = B.leafWord = 0;
	A.nodes = A.tris = B.nodes = B.tris = 0;
	A.t = B.t = 0.0f;
	A.face = B.face = 0;
	A.leafTNear = B.leafTNear = 0.0f;
	A.ray.origin = A.ray.dir = A.invDir = B.ray.origin = B.ray.dir = B.invDir = mk3( 0.0f, 0.0f, 0.0f );
	WorkCursor work = beginWork();

	// both slots take their first unit
	for( int k = 0; k < 2; k++ ) {
		unsigned frame = 0;
		const unsigned slot = nextSlot( P, work, (unsigned) P.nFrames, frame );

		if( slot != PT_NO_WORK ) {
			PixelState st;
			beginPixel( P, st, slot, cnt, frame );
			DualSlot& S = ( k == 0 ) ? A : B;
			S.ray = st.ray;
			startWalkDual<LIGHTS>( P, S );
			storeCold( P, k, st );
		}
	}

	while( __ballot( A.mode != MODE_DONE || B.mode != MODE_DONE ) != 0ull ) {
		// ---- node phase: both slots of every lane ----------------------------------------------------
		// Round 15: what a round costs around nodePhaseDualPipe (profiles/r15/experiments/dual_round_cost.txt).  The test is
		// wave-uniform — the two ballots are the walks' masks, which the phase takes as they are (no cursor select in, none out) —
		// so EXEC is the loop's and nothing is saved or restored around the phase; the slots' cursor, leaf word and tNear are the
		// phase's operands themselves (no zeroed temporaries, no copies back).  With the phase under a scalar branch hipcc keeps
		// the node and face pointers in SGPRs across rounds: the s_load_dwordx4 from kernel-argument memory that stood in front
		// of every node phase's first request, fully exposed, and in front of every leaf phase's, stands in front of the loop.
		// P.nodes is handed over as an opaque scalar, which forces the same where the compiler would not do it by itself; alone
		// that was worth nothing measurable (57.93 against 58.00 ms, the runs overlap), and here it only steers the allocator:
		// without it the chained pathTracingDual<0, true, true> keeps 12 B in scratch instead of 8.
		const unsigned long long walkA = __builtin_amdgcn_ballot_w64( A.mode == MODE_NODE ), walkB = __builtin_amdgcn_ballot_w64( B.mode == MODE_NODE );

		if( ( walkA | walkB ) != 0ull ) {
			const int keep = __popcll( walkA ) + __popcll( walkB ) - P.phPark;
			const f2v oxyA = { A.ray.origin.x, A.ray.origin.y }, oziA = { A.ray.origin.z, A.invDir.z }, ixyA = { A.invDir.x, A.invDir.y };
			const f2v oxyB = { B.ray.origin.x, B.ray.origin.y }, oziB = { B.ray.origin.z, B.invDir.z }, ixyB = { B.invDir.x, B.invDir.y };
			const float4* nodes = P.nodes;
			asm volatile( "" : "+s"( nodes ) );      // opaque: not rematerialised from kernel-argument memory
			__builtin_amdgcn_s_setprio( PT_WALK_PRIO );
			nodePhaseDualPipe( P, nodes, oxyA, oziA, ixyA, A.t, oxyB, oziB, ixyB, B.t, ( keep < 0 ) ? 0 : keep, walkA, walkB, A.cur, B.cur, A.nodes, B.nodes,
			                   A.leafWord, A.leafTNear, B.leafWord, B.leafTNear );
			__builtin_amdgcn_s_setprio( 0 );

			if( A.mode == MODE_NODE ) {
				A.mode = ( A.leafWord != 0 ) ? MODE_LEAF : ( ( A.cur < 0 ) ? MODE_SHADE : MODE_NODE );
			}
			if( B.mode == MODE_NODE ) {
				B.mode = ( B.leafWord != 0 ) ? MODE_LEAF : ( ( B.cur < 0 ) ? MODE_SHADE : MODE_NODE );
			}
		}

		// ---- leaf phase, pooled: the slot that stands on a leaf (A first; B's in the next round) ------------
		{
			const bool leafA = ( A.mode == MODE_LEAF ), leafB = ( B.mode == MODE_LEAF );

			if( leafA || leafB ) {
				const bool useB = !leafA;
				Ray ray;
				ray.origin = useB ? B.ray.origin : A.ray.origin;
				ray.dir = useB ? B.ray.dir : A.ray.dir;
				Hit hit;
				hit.t = useB ? B.t : A.t;
				hit.face = useB ? B.face : A.face;
				const int leafWord = useB ? B.leafWord : A.leafWord;
				const float tNear = useB ? B.leafTNear : A.leafTNear;
				unsigned tests = 0;
				__builtin_amdgcn_s_setprio( PT_WALK_PRIO );
				testLeaf<false, true>( P, leafFace0( leafWord ), leafFace1( leafWord ), ray, tNear, 0.0f, hit, tests );
				__builtin_amdgcn_s_setprio( 0 );

				if( useB ) {
					B.t = hit.t; B.face = hit.face; B.tris += tests; B.leafWord = 0;
					B.mode = ( B.cur < 0 ) ? MODE_SHADE : MODE_NODE;
				}
				else {
					A.t = hit.t; A.face = hit.face; A.tris += tests; A.leafWord = 0;
					A.mode = ( A.cur < 0 ) ? MODE_SHADE : MODE_NODE;
				}
			}
		}

		// ---- shade phase, pooled: the slot that waits for shading (A first); the threshold counts lanes ------
		{
			const bool shadeA = ( A.mode == MODE_SHADE ), shadeB = ( B.mode == MODE_SHADE );
			const int nShade = __popcll( __ballot( shadeA || shadeB ) );
			const bool busy = ( __ballot( A.mode == MODE_NODE || A.mode == MODE_LEAF || B.mode == MODE_NODE || B.mode == MODE_LEAF ) != 0ull );

			if( ( shadeA || shadeB ) && ( nShade >= P.phShade || !busy ) ) {
				const bool useB = !shadeA;
				const int which = useB ? 1 : 0;
				PixelState st;
				loadCold( P, which, st );
				st.ray.origin = useB ? B.ray.origin : A.ray.origin;
				st.ray.dir = useB ? B.ray.dir : A.ray.dir;
				st.dbgNodes += useB ? B.nodes : A.nodes;
				st.dbgTris += useB ? B.tris : A.tris;
				Hit hit;
				hit.t = useB ? B.t : A.t;
				hit.face = useB ? B.face : A.face;
				hit.normal = mk3( 0.0f, 0.0f, 0.0f );
				bool more = true;

				if( shadeStep<BRDF, SHADOW, LIGHTS, false, true, true>( P, lds, st, cnt, hit ) ) {
					finishPixel( P, st );

					if( cnt.nodes > 0x40000000u || cnt.tris > 0x40000000u ) {
						flushCounters( P, cnt );
					}

					unsigned frame = 0;
					const unsigned slot = nextSlot( P, work, (unsigned) P.nFrames, frame );

					if( slot != PT_NO_WORK ) {
						beginPixel( P, st, slot, cnt, frame );
					}
					else {
						more = false;
					}
				}

				storeCold( P, which, st );

				if( useB ) {
					B.nodes = 0; B.tris = 0; B.ray = st.ray;
					if( more ) { startWalkDual<LIGHTS>( P, B ); } else { B.mode = MODE_DONE; B.cur = -1; }
				}
				else {
					A.nodes = 0; A.tris = 0; A.ray = st.ray;
					if( more ) { startWalkDual<LIGHTS>( P, A ); } else { A.mode = MODE_DONE; A.cur = -1; }
				}
			}
		}
	}

	flushCounters( P, cnt );
}
#endif   // PT_NODE_PHASE_ASM
