# The translation units of the library, in ONE place: csrc/Makefile builds libm4ri_hip.so from them, tools/Makefile the development
# library (-DGF2K_DEV_VARIANTS).  A new file is added here and nowhere else; one in a subdirectory is listed with its directory.
LIB_SRC := gf2_kernels.hip gf2_elim.hip gf2_elim_batch.hip gf2_ple.hip gf2_trsm.hip gf2_nullspace.hip gf2_blocks.hip \
           gather/gf2_gather.hip gather/gather_host.cpp weight/gf2_weight.hip weight/weight_host.cpp wht/gf2_wht.hip wht/wht_host.cpp \
           bkw/gf2_bkw.hip bkw/bkw_host.cpp cover/gf2_cover.hip cover/cover_host.cpp lf2/gf2_lf2.hip lf2/lf2_host.cpp \
           draw/gf2_draw.hip draw/draw_host.cpp join/gf2_join.hip join/join_host.cpp sums/gf2_sums.hip sums/sums_host.cpp \
           near/gf2_near.hip near/near_host.cpp unique/gf2_unique.hip unique/unique_host.cpp find/gf2_find.hip find/find_host.cpp \
           join_rows/gf2_join_rows.hip join_rows/join_rows_host.cpp \
           runtime_host.cpp mul_plan_host.cpp mul_dev_host.cpp m4ri_hip_api.cpp elim_host.cpp mzd_host.cpp gf2_small_host.cpp \
           ple_host.cpp trsm_host.cpp nullspace_host.cpp blocks_host.cpp elim_batch_host.cpp
LIB_HDR := gf2_kernels.h gf2_dev_words.h gf2_env.h gf2_variants.h gf2_lpn.inc strassen/gf2_merge4.inc api_internal.h dev_args.h mul_plan.h gather/gather_plan.h gather/gf2_gather.h \
           weight/weight_plan.h weight/gf2_weight.h wht/wht_plan.h wht/gf2_wht.h bkw/bkw_plan.h bkw/gf2_bkw.h cover/cover_plan.h cover/gf2_cover.h lf2/lf2_plan.h lf2/gf2_lf2.h \
           draw/draw_plan.h draw/gf2_draw.h draw/philox.h join/join_plan.h join/gf2_join.h join/gf2_join_select.inc sums/sums_plan.h sums/gf2_sums.h near/near_plan.h near/gf2_near.h \
           unique/unique_plan.h unique/gf2_unique.h ../../include/m4ri_hip_unique.h find/find_plan.h find/gf2_find.h ../../include/m4ri_hip_find.h \
           join_rows/join_rows_plan.h join_rows/gf2_join_rows.h ../../include/m4ri_hip_join_rows.h \
           ../../include/m4ri_hip.h ../../include/m4ri_hip_gather.h ../../include/m4ri_hip_weight.h ../../include/m4ri_hip_wht.h \
           ../../include/m4ri_hip_bkw.h ../../include/m4ri_hip_cover.h ../../include/m4ri_hip_lf2.h ../../include/m4ri_hip_draw.h \
           ../../include/m4ri_hip_join.h ../../include/m4ri_hip_join_select.h ../../include/m4ri_hip_sums.h ../../include/m4ri_hip_near.h
