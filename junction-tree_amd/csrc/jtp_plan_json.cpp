// Planner, unit 6 of 6 (jtp_plan_build.h has the map): the plan as JSON (jtp_plan_describe, the tests, tools/plan_digest.py).
#include "jtp_plan_build.h"

namespace {
template <typename It>
void json_list(std::ostringstream &o, It a, It b) {
    o << "[";
    for (It i = a; i != b; ++i) {
        if (i != a) o << ",";
        o << (long long)*i;
    }
    o << "]";
}
template <typename V>
void json_vec(std::ostringstream &o, const V &v) { json_list(o, v.begin(), v.end()); }

void json_msg(std::ostringstream &o, const JtMsg &m, int nF) {
    o << "{\"off\":" << m.off << ",\"npart\":" << m.npart << ",\"pstride\":" << m.pstride
      << ",\"nfree\":" << m.nfree << ",\"lds_off\":" << m.lds_off << ",\"e_w\":";
    json_list(o, m.e_w, m.e_w + 2);
    o << ",\"t_w\":";
    json_list(o, m.t_w, m.t_w + 8);
    o << ",\"red_e\":" << m.red_e << ",\"red_lane\":" << m.red_lane << ",\"red_wave\":" << m.red_wave
      << ",\"e_dep\":" << m.e_dep << ",\"same_launch\":" << m.same_launch << ",\"fixed\":" << m.fixed << ",\"f_w\":";
    json_list(o, m.f_w, m.f_w + nF);
    o << ",\"f_p\":";
    json_list(o, m.f_p, m.f_p + nF);
    o << ",\"free_pos\":";
    json_list(o, m.free_pos, m.free_pos + m.nfree);
    o << "}";
}
}  // namespace

static std::string json_escape(const std::string &s) {
    std::string o;
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\', o += c;
        else if ((unsigned char)c < 0x20) o += ' ';
        else o += c;
    }
    return o;
}

void jtp_plan_to_json(HostPlan &hp, bool with_tasks) {
    std::ostringstream o;
    o << "{\"version\":1,\"dtype\":" << hp.dtype << ",\"VEC\":" << hp.VEC << ",\"EB\":" << hp.EB << ",\"TB\":" << hp.TB
      << ",\"n_cliques\":" << hp.n_cliques << ",\"n_ranks\":" << hp.n_ranks << ",\"rank\":" << hp.rank
      << ",\"root\":" << hp.root << ",\"arena_elems\":" << hp.arena_elems << ",\"msg_doubles\":" << hp.msg_doubles
      << ",\"dbg_base\":" << hp.dbg_base << ",\"max_lds\":" << hp.max_lds << ",\"alg_bytes\":" << (long long)hp.alg_bytes
      << ",\"staging_bytes\":" << (long long)hp.staging_bytes << ",\"table_bytes\":" << (long long)hp.table_bytes
      << ",\"compact\":" << (hp.compact ? 1 : 0) << ",\"tmix\":" << (hp.tmix ? 1 : 0) << ",\"host_table_elems\":" << (long long)hp.host_table_elems
      << ",\"multiset\":" << (hp.multiset ? 1 : 0) << ",\"alg_table_bytes\":" << (long long)hp.alg_table_bytes
      << ",\"alg_msg_bytes\":" << (long long)hp.alg_msg_bytes
      << ",\"n_messages\":" << hp.n_messages << ",\"n_tasks\":" << hp.tasks.size()
      << ",\"n_blocks\":" << hp.blocks.size() << ",\"tmix_compact\":" << (hp.tmix_compact ? 1 : 0) << ",\"lean\":" << (hp.lean ? 1 : 0) << ",\"has_unit\":" << (hp.has_unit ? 1 : 0)
      << ",\"lean_refused\":\"" << json_escape(hp.lean_refused) << "\",\"fix_doubles\":" << hp.fix_doubles << ",\"scratch_elems\":" << hp.scratch_elems << ",\"alg_bytes_full\":" << (long long)hp.alg_bytes_full;
    o << ",\"keep\":{\"budget_bytes\":" << (long long)hp.keep_budget << ",\"collect_bytes\":" << (long long)hp.keep_bytes[0]
      << ",\"distribute_bytes\":" << (long long)hp.keep_bytes[1] << ",\"levels\":";
    json_vec(o, hp.keep_levels);
    o << "}";
    o << ",\"statics\":[";
    for (size_t i = 0; i < hp.statics.size(); ++i) {
        const PStatic &st = hp.statics[i];
        if (i) o << ",";
        o << "{\"pnode\":" << st.pnode << ",\"nbits\":" << st.nbits << ",\"off\":" << st.off << ",\"vars\":";
        json_vec(o, st.vars);
        o << ",\"pos\":";
        json_vec(o, st.pos);
        o << ",\"nb\":";
        json_vec(o, st.nb);
        o << "}";
    }
    o << "],\"pnodes\":[";
    for (size_t i = 0; i < hp.pn.size(); ++i) {
        const PNode &p = hp.pn[i];
        if (i) o << ",";
        o << "{\"real\":" << p.real << ",\"parent\":" << p.parent << ",\"psep\":" << p.psep << ",\"depth\":" << p.depth
          << ",\"owner\":" << p.owner << ",\"nbits\":" << p.nbits << ",\"arena_off\":" << p.arena_off
          << ",\"phys_elems\":" << p.phys_elems << ",\"pad_mask\":" << p.pad_mask << ",\"tmix\":" << (p.tmix ? 1 : 0) << ",\"trow\":" << p.trow
          << ",\"tpad_mask\":" << p.tpad_mask << ",\"tsplit\":" << p.tsplit << ",\"tsplit_lb\":" << p.tsplit_lb << ",\"tmap_off\":" << p.tmap_off << ",\"layout\":" << p.layout << ",\"collect_task\":" << p.collect_task << ",\"distribute_task\":" << p.distribute_task
          << ",\"unit\":" << (p.unit ? 1 : 0) << ",\"stat\":" << p.stat << ",\"cover\":";
        json_vec(o, p.cover);
        o << ",\"down_tasks\":";
        json_vec(o, p.down_tasks);
        if (hp.tmix || p.unit) {
            o << ",\"tmap\":";
            json_vec(o, p.tmap);
            o << ",\"vmap\":";
            json_vec(o, p.vmap);
        }
        o << ",\"bitw\":";
        json_vec(o, p.bitw);
        o << ",\"group_mask\":";
        json_vec(o, p.group_mask);
        o << ",\"group_pos\":";
        json_vec(o, p.group_pos);
        o << ",\"group_card\":";
        json_vec(o, p.group_card);
        {
            std::vector<int> cards;
            for (int v : p.vars) cards.push_back(hp.card[v]);
            o << ",\"card\":";
            json_vec(o, cards);
        }
        o << ",\"vars\":";
        json_vec(o, p.vars);
        o << ",\"pos\":";
        json_vec(o, p.pos);
        o << ",\"nb\":";
        json_vec(o, p.nb);
        o << ",\"children\":";
        json_vec(o, p.children);
        o << "}";
    }
    o << "],\"pack\":[";                      // host <-> device conversion records of the real cliques (host variable order)
    for (size_t i = 0; i < hp.pack.size(); ++i) {
        const JtPackDesc &pd = hp.pack[i];
        if (i) o << ",";
        o << "{\"pos\":";
        json_list(o, pd.pos, pd.pos + pd.nvars);
        o << ",\"nb\":";
        json_list(o, pd.nb, pd.nb + pd.nvars);
        o << ",\"card\":";
        json_list(o, pd.card, pd.card + pd.nvars);
        o << ",\"dstride\":";
        json_list(o, pd.dstride, pd.dstride + pd.nvars);
        o << ",\"dmod\":";
        json_list(o, pd.dmod, pd.dmod + pd.nvars);
        o << ",\"split_var\":" << pd.split_var << ",\"split_lb\":" << pd.split_lb << ",\"split_ds2\":" << pd.split_ds2 << ",\"split_mod2\":" << pd.split_mod2;
        o << ",\"phys_elems\":" << pd.phys_elems << "}";
    }
    o << "],\"pseps\":[";
    for (size_t i = 0; i < hp.ps.size(); ++i) {
        const PSep &s = hp.ps[i];
        if (i) o << ",";
        o << "{\"node\":" << s.node << ",\"child\":" << s.child << ",\"parent\":" << s.parent << ",\"nbits\":" << s.nbits
          << ",\"up_npart\":" << s.up_npart << ",\"dn_npart\":" << s.dn_npart << ",\"up_off\":" << s.up_off
          << ",\"dn_off\":" << s.dn_off << ",\"up_roff\":" << s.up_roff << ",\"dn_roff\":" << s.dn_roff
          << ",\"up_rnpart\":" << s.up_rnpart << ",\"dn_rnpart\":" << s.dn_rnpart
          << ",\"up_red_task\":" << s.up_red_task << ",\"dn_red_task\":" << s.dn_red_task << ",\"dn_task\":" << s.dn_task << ",\"vars\":";
        json_vec(o, s.vars);
        o << ",\"pos\":";
        json_vec(o, s.pos);
        o << ",\"nb\":";
        json_vec(o, s.nb);
        o << "}";
    }
    o << "],\"launches\":[";
    for (size_t i = 0; i < hp.launches.size(); ++i) {
        const Launch &L = hp.launches[i];
        if (i) o << ",";
        o << "{\"phase\":" << L.phase << ",\"level\":" << L.level << ",\"variant\":" << L.variant
          << ",\"nblocks\":" << L.nblocks << ",\"blk_off\":" << L.blk_off << ",\"lds_bytes\":" << L.lds_bytes
          << ",\"alg_bytes\":" << (long long)L.alg_bytes << ",\"tasks\":";
        json_vec(o, L.tasks);
        o << "}";
    }
    o << "],\"steps\":[";
    for (size_t i = 0; i < hp.steps.size(); ++i) {
        if (i) o << ",";
        o << "[" << hp.steps[i].kind << "," << hp.steps[i].first << "," << hp.steps[i].count << "]";
    }
    o << "],\"sync_words\":" << hp.sync_words << ",\"segments\":[";
    for (size_t i = 0; i < hp.segments.size(); ++i) {
        const Segment &g = hp.segments[i];
        if (i) o << ",";
        o << "{\"phase\":" << g.phase << ",\"first_launch\":" << g.first_launch << ",\"n_launch\":" << g.n_launch
          << ",\"blk_off\":" << g.blk_off << ",\"nblocks\":" << g.nblocks << ",\"lds_bytes\":" << g.lds_bytes
          << ",\"ticket_idx\":" << g.ticket_idx << "}";
    }
    o << "],\"flow_steps\":[";
    for (size_t i = 0; i < hp.flow_steps.size(); ++i) {
        if (i) o << ",";
        o << "[" << hp.flow_steps[i].kind << "," << hp.flow_steps[i].first << "," << hp.flow_steps[i].count << "]";
    }
    o << "],\"comm\":[";
    for (size_t i = 0; i < hp.comm.size(); ++i) {
        const CommOp &c = hp.comm[i];
        if (i) o << ",";
        o << "{\"send\":" << c.send << ",\"psep\":" << c.psep << ",\"up\":" << c.up << ",\"peer\":" << c.peer
          << ",\"off\":" << c.off << ",\"count\":" << c.count << "}";
    }
    o << "]";
    o << ",\"sample\":{\"refused\":\"" << json_escape(hp.sample_refused) << "\",\"depths\":[";
    for (size_t i = 0; i < hp.sample_depths.size(); ++i) {
        if (i) o << ",";
        std::vector<int> cl;
        for (int k : hp.sample_depths[i]) cl.push_back(hp.sample[k].clique);
        json_vec(o, cl);
    }
    o << "],\"cliques\":[";
    for (size_t i = 0; i < hp.sample.size(); ++i) {
        const SampleClique &sc = hp.sample[i];
        if (i) o << ",";
        o << "{\"clique\":" << sc.clique << ",\"depth\":" << sc.depth << ",\"parent\":" << hp.parent_clique[sc.clique] << ",\"R\":" << sc.R << ",\"K\":";
        json_vec(o, sc.K);
        o << ",\"F\":";
        json_vec(o, sc.F);
        o << "}";
    }
    o << "]}";
    if (hp.scaled) {                  // (plans without JTP_SCALED describe as they always did)
        o << ",\"scaled\":1,\"rescale\":[";
        for (size_t i = 0; i < hp.rescale.size(); ++i) {
            const JtRescale &r = hp.rescale[i];
            if (i) o << ",";
            o << "{\"off\":" << r.off << ",\"count\":" << r.count << ",\"slot\":" << r.slot << "}";
        }
        o << "]";
    }
    if (with_tasks) {
        o << ",\"tasks\":[";
        for (size_t t = 0; t < hp.tasks.size(); ++t) {
            const JtTask &tk = hp.tasks[t];
            if (t) o << ",";
            o << "{\"pnode\":" << tk.pnode << ",\"kind\":" << tk.kind << ",\"mode\":" << tk.mode << ",\"unit\":" << tk.unit << ",\"setb\":" << tk.setb << ",\"esum\":" << tk.esum << ",\"variant\":" << hp.task_variant[t] << ",\"psi_off\":" << tk.psi_off
              << ",\"bel_off\":" << tk.bel_off << ",\"nbits\":" << tk.nbits << ",\"real_bits\":" << tk.real_bits << ",\"nF\":" << tk.nF << ",\"nA\":" << tk.nA
              << ",\"nR\":" << tk.nR << ",\"settle\":" << tk.settle << ",\"keep_rows\":" << tk.keep_rows << ",\"tmap_off\":" << tk.tmap_off << ",\"fold\":" << tk.fold << ",\"lean_off\":" << tk.lean_off << ",\"vgroups\":" << tk.vgroups << ",\"out_run\":" << tk.out_run << ",\"n_in\":" << tk.n_in << ",\"n_out\":" << tk.n_out
              << ",\"lds_bytes\":" << tk.lds_bytes << ",\"first_x\":";
            json_list(o, tk.first_x, tk.first_x + 8);
            o << ",\"f_x\":";
            json_list(o, tk.f_x, tk.f_x + tk.nF);
            o << ",\"f_lx\":";
            json_list(o, tk.f_lx, tk.f_lx + tk.nF);
            o << ",\"loop_pos\":";
            json_list(o, tk.loop_pos, tk.loop_pos + tk.nA + tk.nR);
            o << ",\"total\":" << tk.total << ",\"itab_lds\":" << tk.itab_lds << ",\"itab\":[";
            for (int i = 0; i < tk.total; ++i) {
                if (i) o << ",";
                json_list(o, hp.itab.begin() + tk.itab_off + (size_t)i * JT_NCOL, hp.itab.begin() + tk.itab_off + (size_t)(i + 1) * JT_NCOL);
            }
            o << "],\"in\":[";
            for (int k = 0; k < tk.n_in; ++k) {
                if (k) o << ",";
                json_msg(o, tk.msg[k], tk.nF);
            }
            o << "],\"out\":[";
            for (int k = 0; k < tk.n_out; ++k) {
                if (k) o << ",";
                json_msg(o, tk.msg[JT_MAX_IN + k], tk.nF);
            }
            o << "]";
            if (tk.lean_off > 0 && (size_t)tk.lean_off + sizeof(JtLean) / 4 <= hp.itab.size()) {      // (the record as the kernel reads it)
                o << ",\"lean\":";
                json_list(o, hp.itab.begin() + tk.lean_off, hp.itab.begin() + tk.lean_off + sizeof(JtLean) / 4);
            }
            o << "}";
        }
        o << "],\"blocks\":[";
        for (size_t b = 0; b < hp.blocks.size(); ++b) {
            if (b) o << ",";
            const JtBlock &k = hp.blocks[b];
            o << "[" << k.task << "," << hp.block_chunk[b] << "," << k.xF;
            for (int i = 0; i < JT_MAX_MSG; ++i) o << "," << k.gbase[i];
            for (int i = 0; i < JT_MAX_OUT; ++i) o << "," << k.pnum[i];
            o << "," << k.psi_x0;
            for (int i = 0; i < 8; ++i) o << "," << k.first_x[i];
            o << "," << k.lxF << "," << k.flags;
            o << "]";
        }
        o << "],\"init_blocks\":[";
        bool first_init = true;
        for (int m = 0; m < 2; ++m)
            for (size_t b = 0; b < hp.init_blocks[m].size(); ++b) {
                if (!first_init) o << ",";
                first_init = false;
                const JtBlock &k = hp.init_blocks[m][b];
                o << "[" << k.task << "," << hp.init_chunk[m][b] << "," << k.xF;
                for (int i = 0; i < JT_MAX_MSG; ++i) o << "," << k.gbase[i];
                for (int i = 0; i < JT_MAX_OUT; ++i) o << "," << k.pnum[i];
                o << "," << k.psi_x0;
                for (int i = 0; i < 8; ++i) o << "," << k.first_x[i];
                o << "," << k.lxF << "," << k.flags;
                o << "]";
            }
        o << "]";
    }
    o << "}";
    hp.json = o.str();
}
