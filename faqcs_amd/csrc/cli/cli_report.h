// cli_report.h -- what `faqcs_mi` writes about a run: QC.stats.txt (FaQCs.cpp:759-1034), the --debug tables (plot.cpp:540-733), the R
// script of the PDF report and the helper process that runs it.
#pragma once
#include "cli_options.h"

namespace {
std::string fmt(const char *f, ...)
{
    char buf[512]; va_list ap; va_start(ap, f); vsnprintf(buf, sizeof(buf), f, ap); va_end(ap); return buf;
}
std::string pct(double a, double b) { return fmt("%.2f", (100.0 * a) / b); }
std::string f2(double x, int prec = 2) { return fmt("%.*f", prec, x); }

void adapter_lines(std::string &out, const uint64_t *fs, std::map<std::string, std::pair<uint64_t, uint64_t>> &ast)
{
    std::vector<std::pair<uint64_t, std::string>> v;
    for (auto &kv : ast) v.emplace_back(kv.second.first, kv.first);
    std::sort(v.begin(), v.end());
    for (auto it = v.rbegin(); it != v.rend(); ++it) {
        const auto &st = ast[it->second];
        out += "    " + it->second + " " + std::to_string(st.first) + " reads (" + pct((double)st.first, (double)fs[FAQCS_TOTAL_NUMBER]) + " %) " +
               std::to_string(st.second) + " bases (" + pct((double)st.second, (double)fs[FAQCS_TOTAL_LENGTH]) + " %)\n";
    }
}

std::string stats_text(const Opt &o, const uint64_t *fs, std::map<std::string, std::pair<uint64_t, uint64_t>> &ast, int quality)
{
    auto T = [&](int k) { return (unsigned long long)fs[k]; };
    auto D = [&](int k) { return (double)fs[k]; };
    std::string s;
    if (o.qc_only) {
        s += "\n";
        s += fmt("Reads #: %llu\n", T(FAQCS_TOTAL_COUNT));
        s += fmt("Total bases: %llu\n", T(FAQCS_TOTAL_LENGTH));
        s += "Reads Length: " + f2((double)((float)fs[FAQCS_TOTAL_LENGTH] / (float)fs[FAQCS_TOTAL_COUNT])) + "\n";
        s += fmt("Processed %llu reads for quality check only\n", T(FAQCS_TOTAL_NUMBER));
        s += fmt("  Reads length < %u bp: %llu (", o.min_len, T(FAQCS_READ_LENGTH)) + pct(D(FAQCS_READ_LENGTH), D(FAQCS_TOTAL_NUMBER)) + " %)\n";
        s += fmt("  Reads have %u continuous base \"N\": %llu (", o.max_poly_n, T(FAQCS_READ_NN)) + pct(D(FAQCS_READ_NN), D(FAQCS_TOTAL_NUMBER)) + " %)\n";
        s += "  Low complexity Reads  (>" + f2((double)o.lc * 100.0) + fmt("%% mono/di-nucleotides): %llu (", T(FAQCS_READ_LOW_COMPLEXITY)) +
             pct(D(FAQCS_READ_LOW_COMPLEXITY), D(FAQCS_TOTAL_NUMBER)) + " %)\n";
        s += "  Reads < average quality " + f2((double)o.average_quality) + fmt(": %llu (", T(FAQCS_READ_AVG_Q)) + pct(D(FAQCS_READ_AVG_Q), D(FAQCS_TOTAL_NUMBER)) + " %)\n";
        if (o.filter_phiX) s += fmt("  Reads hits to phiX sequence: %llu (", T(FAQCS_READ_PHIX)) + pct(D(FAQCS_READ_PHIX), D(FAQCS_TOTAL_NUMBER)) + " %)\n";
        if (o.filter_adapter) {
            s += fmt("  Reads with Adapters/Primers: %llu (", T(FAQCS_READ_ADAPTER)) + pct(D(FAQCS_READ_ADAPTER), D(FAQCS_TOTAL_NUMBER)) + " %)\n";
            adapter_lines(s, fs, ast);
        }
        return s;
    }
    const double tn = D(FAQCS_TOTAL_NUMBER), tl = D(FAQCS_TOTAL_LENGTH), ttn = D(FAQCS_TOTAL_TRIMMED_NUMBER), ttl = D(FAQCS_TOTAL_TRIMMED_LENGTH);
    s += "Before Trimming\n";
    s += fmt("Reads #: %llu\n", T(FAQCS_TOTAL_NUMBER));
    s += fmt("Total bases: %llu\n", T(FAQCS_TOTAL_LENGTH));
    s += "Reads Length: " + f2((double)((float)fs[FAQCS_TOTAL_LENGTH] / (float)fs[FAQCS_TOTAL_NUMBER])) + "\n";
    s += "\nAfter Trimming\n";
    s += fmt("Reads #: %llu (", T(FAQCS_TOTAL_TRIMMED_NUMBER)) + pct(ttn, tn) + " %)\n";
    s += fmt("Total bases: %llu (", T(FAQCS_TOTAL_TRIMMED_LENGTH)) + pct(ttl, tl) + " %)\n";
    if (fs[FAQCS_TOTAL_TRIMMED_NUMBER] > 0) s += "Mean Reads Length: " + f2((double)((float)fs[FAQCS_TOTAL_TRIMMED_LENGTH] / (float)fs[FAQCS_TOTAL_TRIMMED_NUMBER])) + "\n";
    else s += "Mean Reads Length: 0\n";
    if (!o.in1.empty()) {
        const double prn = D(FAQCS_PAIRED_READ_NUMBER), pbl = D(FAQCS_PAIRED_BASE_LENGTH);
        s += fmt("  Paired Reads #: %llu (", T(FAQCS_PAIRED_READ_NUMBER)) + pct(prn, ttn) + " %)\n";
        s += fmt("  Paired total bases: %llu (", T(FAQCS_PAIRED_BASE_LENGTH)) + pct(pbl, ttl) + " %)\n";
        s += fmt("  Unpaired Reads #: %llu (", T(FAQCS_TOTAL_TRIMMED_NUMBER) - T(FAQCS_PAIRED_READ_NUMBER)) + pct(ttn - prn, ttn) + " %)\n";
        s += fmt("  Unpaired total bases: %llu (", T(FAQCS_TOTAL_TRIMMED_LENGTH) - T(FAQCS_PAIRED_BASE_LENGTH)) + pct(ttl - pbl, ttl) + " %)\n";
    }
    s += fmt("\nDiscarded reads #: %llu (", T(FAQCS_TOTAL_NUMBER) - T(FAQCS_TOTAL_TRIMMED_NUMBER)) + pct(tn - ttn, tn) + " %)\n";
    s += fmt("Trimmed bases: %llu (", T(FAQCS_TOTAL_LENGTH) - T(FAQCS_TOTAL_TRIMMED_LENGTH)) + pct(tl - ttl, tl) + " %)\n";
    s += fmt("  Reads Filtered by length cutoff (%u bp): %llu (", o.min_len, T(FAQCS_READ_LENGTH)) + pct(D(FAQCS_READ_LENGTH), tn) + " %)\n";
    s += fmt("  Bases Filtered by length cutoff: %llu (", T(FAQCS_BASE_LENGTH)) + pct(D(FAQCS_BASE_LENGTH), tl) + " %)\n";
    s += fmt("  Reads Filtered by continuous base \"N\" (%u): %llu (", o.max_poly_n, T(FAQCS_READ_NN)) + pct(D(FAQCS_READ_NN), tn) + " %)\n";
    s += fmt("  Bases Filtered by continuous base \"N\": %llu (", T(FAQCS_BASE_NN)) + pct(D(FAQCS_BASE_NN), tl) + " %)\n";
    s += "  Reads Filtered by low complexity ratio (" + f2((double)o.lc, 1) + fmt("): %llu (", T(FAQCS_READ_LOW_COMPLEXITY)) + pct(D(FAQCS_READ_LOW_COMPLEXITY), tn) + " %)\n";
    s += fmt("  Bases Filtered by low complexity ratio: %llu (", T(FAQCS_BASE_LOW_COMPLEXITY)) + pct(D(FAQCS_BASE_LOW_COMPLEXITY), tl) + " %)\n";
    if (o.average_quality > 0.0f) {
        s += "  Reads Filtered by avg quality (" + f2((double)o.average_quality) + fmt("): %llu (", T(FAQCS_READ_AVG_Q)) + pct(D(FAQCS_READ_AVG_Q), tn) + " %)\n";
        s += fmt("  Bases Filtered by avg quality: %llu (", T(FAQCS_BASE_AVG_Q)) + pct(D(FAQCS_BASE_AVG_Q), tl) + " %)\n";
    }
    if (o.filter_phiX) {
        s += fmt("  Reads Filtered by phiX sequence: %llu (", T(FAQCS_READ_PHIX)) + pct(D(FAQCS_READ_PHIX), tn) + " %)\n";
        s += fmt("  Bases Filtered by phiX sequence: %llu (", T(FAQCS_BASE_PHIX)) + pct(D(FAQCS_BASE_PHIX), tl) + " %)\n";
    }
    s += "  Reads Trimmed by quality (" + f2((double)(float)quality, 1) + fmt("): %llu (", T(FAQCS_READ_QUAL_TRIM)) + pct(D(FAQCS_READ_QUAL_TRIM), tn) + " %)\n";
    s += fmt("  Bases Trimmed by quality: %llu (", T(FAQCS_BASE_QUAL_TRIM)) + pct(D(FAQCS_BASE_QUAL_TRIM), tl) + " %)\n";
    if (o.trim_5 > 0) s += fmt("  Reads Trimmed with %u bp from 5' end\n", o.trim_5);
    if (o.trim_3 > 0) s += fmt("  Reads Trimmed with %u bp from 3' end\n", o.trim_3);
    if (o.filter_adapter) {
        s += fmt("  Reads Trimmed with Adapters/Primers: %llu (", T(FAQCS_READ_ADAPTER)) + pct(D(FAQCS_READ_ADAPTER), tn) + " %)\n";
        s += fmt("  Bases Trimmed with Adapters/Primers: %llu (", T(FAQCS_BASE_ADAPTER)) + pct(D(FAQCS_BASE_ADAPTER), tl) + " %)\n";
        adapter_lines(s, fs, ast);
    }
    if (o.replace_N) s += fmt("\nN base random substitution: A %llu, T %llu, C %llu, G %llu\n", T(FAQCS_N_TO_A), T(FAQCS_N_TO_T), T(FAQCS_N_TO_C), T(FAQCS_N_TO_G));
    return s;
}

void put_file(const std::string &path, const std::string &text) { FILE *f = fopen(path.c_str(), "w"); if (f) { fwrite(text.data(), 1, text.size(), f); fclose(f); } }

// (cnt, nk, pts: the run's k-mer count histogram and rarefaction points, Run::kmer_results)
void write_tables(const Opt &o, const faqcs_layout &L, const uint64_t *c, uint32_t R, const std::vector<uint64_t> &cnt, const std::vector<uint64_t> &nk,
                  const std::vector<faqcs_rarefaction> &pts)
{
    const std::string d = o.output_dir + "/", p = o.prefix;
    const uint32_t rows_pre = faqcs_counter_rows(c + L.pre_qual, R, FAQCS_NQ), rows_post = faqcs_counter_rows(c + L.post_qual, R, FAQCS_NQ);
    auto matrix = [&](const std::string &name, const uint64_t *m, uint32_t rows, uint32_t cols) { // plot.cpp:613-640
        if (!rows) return;
        std::string t;
        for (uint32_t r = 0; r < rows; ++r) for (uint32_t k = 0; k < cols; ++k) { t += std::to_string(m[(size_t)r * cols + k]); t += k + 1 < cols ? '\t' : '\n'; }
        put_file(d + name, t);
    };
    matrix("qa." + p + ".quality.matrix", c + L.pre_qual, rows_pre, FAQCS_NQ);
    matrix(p + ".quality.matrix", c + L.post_qual, rows_post, FAQCS_NQ);
    matrix("qa." + p + ".base.matrix", c + L.pre_base, rows_pre, FAQCS_NBASE);
    matrix(p + ".base.matrix", c + L.post_base, rows_post, FAQCS_NBASE);
    auto qhist = [&](const std::string &name, const uint64_t *rh, const uint64_t *bh) { // plot.cpp:642-663
        std::string t = "Score\treadsNum\treadsBases\n";
        for (int i = FAQCS_NQ - 1; i >= 0; --i) t += fmt("%d\t%llu\t%llu\n", i, (unsigned long long)rh[i], (unsigned long long)bh[i]);
        put_file(d + name, t);
    };
    qhist("qa." + p + ".for_qual_histogram.txt", c + L.pre_read_qhist, c + L.pre_base_qhist);
    qhist(p + ".for_qual_histogram.txt", c + L.post_read_qhist, c + L.post_base_qhist);
    auto comp = [&](const std::string &name, const uint64_t *m) { // plot.cpp:540-611
        static const char *kind[6] = {"A", "T", "C", "G", "N", "GC"};
        std::string t;
        for (int k = 0; k < 6; ++k) for (uint32_t i = 0; i < FAQCS_NCOMP_BIN; ++i) { const uint64_t v = m[(size_t)i * 6 + k]; if (v) t += fmt("%s\t%.2f\t%llu\n", kind[k], i * 0.01, (unsigned long long)v); }
        put_file(d + name, t);
    };
    comp("qa." + p + ".base_content.txt", c + L.pre_comp);
    comp(p + ".base_content.txt", c + L.post_comp);
    auto lenhist = [&](const std::string &name, const uint64_t *h) { // plot.cpp:665-681
        uint32_t size = 0;
        for (uint32_t i = 0; i <= R; ++i) if (h[i]) size = i + 1;
        std::string t;
        for (uint32_t i = 1; i < size; ++i) t += fmt("%u\t%llu\n", i, (unsigned long long)h[i]);
        put_file(d + name, t);
    };
    lenhist("qa." + p + ".length_count.txt", c + L.pre_len_hist);
    lenhist(p + ".length_count.txt", c + L.post_len_hist);
    if (!cnt.empty()) { // plot.cpp:683-733
        std::string t;
        for (size_t i = 0; i < cnt.size(); ++i) t += fmt("%llu %llu\n", (unsigned long long)cnt[i], (unsigned long long)nk[i]);
        put_file(d + p + ".kmerH.txt", t);
        t.clear();
        uint64_t lastn = 0;
        for (size_t i = 0; i < pts.size(); ++i) { t += fmt("%llu\t%llu\t%llu\n", (unsigned long long)(pts[i].num_seq - lastn), (unsigned long long)pts[i].distinct_kmer, (unsigned long long)pts[i].total_kmer); lastn = pts[i].num_seq; }
        put_file(d + p + ".Kmercount.txt", t);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The PDF report (plot.cpp:93-515: the reference pipes an R script into `R --vanilla --silent --slave`, then deletes the tables
// unless --debug).  Same process contract here -- same command, same tables on disk while R runs, same PDF name -- with a script
// written for this repository (the reference's script text is not reproduced): one page per plot of the reference's report.
// ---------------------------------------------------------------------------------------------------------------------
std::string r_quote(const std::string &s)
{
    std::string q = "\"";
    for (char ch : s) { if (ch == '\\' || ch == '"') q += '\\'; q += ch; }
    return q + "\"";
}

std::string report_script(const Opt &o)
{
    const std::string d = o.output_dir + "/", p = o.prefix;
    std::string s;
    s += "options(warn = -1)\n";
    s += "pdf_file <- " + r_quote(o.plots_file) + "\n";
    s += "stats_file <- " + r_quote(o.stats_file) + "\n";
    s += "pre <- function(name) file.path(" + r_quote(o.output_dir) + ", paste0(\"qa.\", " + r_quote(p) + ", \".\", name))\n";
    s += "post <- function(name) file.path(" + r_quote(o.output_dir) + ", paste0(" + r_quote(p) + ", \".\", name))\n";
    s += std::string("qc_only <- ") + (o.qc_only ? "TRUE" : "FALSE") + "\n";
    s += R"R(
have <- function(f) file.exists(f) && file.info(f)$size > 0
page <- function(expr) try(expr, silent = TRUE)
both <- function(name) c(pre(name), post(name))[c(have(pre(name)), have(post(name)))]
label <- function(f) if (grepl("/qa\\.[^/]*$", f)) "input reads" else if (qc_only) "reads (QC only)" else "trimmed reads"

pdf(file = pdf_file, width = 12, height = 7)

# 1. the statistics text
page({
  txt <- readLines(stats_file)
  par(family = "mono", mar = c(1, 1, 3, 1))
  plot(0:1, 0:1, type = "n", axes = FALSE, xlab = "", ylab = "")
  step <- min(0.035, 0.95 / max(1, length(txt)))
  for (i in seq_along(txt)) text(0.02, 1 - step * (i - 1), txt[i], adj = 0, cex = 0.8)
  title("QC statistics")
  par(family = "", mar = c(5, 4, 4, 2) + 0.1)
})

# 2. read length histograms
page({
  fs <- both("length_count.txt")
  if (length(fs)) {
    par(mfrow = c(1, length(fs)))
    for (f in fs) {
      t <- read.table(f, header = FALSE, col.names = c("len", "n"))
      barplot(t$n / 1e6, names.arg = t$len, xlab = "length (bases)", ylab = "reads (millions)", main = label(f), border = NA, col = "steelblue")
    }
    par(mfrow = c(1, 1))
    mtext("Read length histogram", outer = TRUE, line = -1.5, font = 2)
  }
})

# 3. composition of the reads: GC, then A, T, C, G, N
content <- function(f) read.table(f, header = FALSE, col.names = c("kind", "pct", "n"), stringsAsFactors = FALSE)
page({
  fs <- both("base_content.txt")
  if (length(fs)) {
    par(mfrow = c(1, length(fs)))
    for (f in fs) {
      t <- content(f); g <- t[t$kind == "GC", ]
      if (nrow(g)) {
        m <- sum(g$pct * g$n) / sum(g$n)
        plot(g$pct, g$n / 1e3, type = "h", xlim = c(0, 100), xlab = "GC (%)", ylab = "reads (thousands)", main = label(f), col = "darkgreen")
        legend("topright", legend = sprintf("mean %.2f %%", m), bty = "n")
      }
    }
    par(mfrow = c(1, 1))
    mtext("GC content of the reads", outer = TRUE, line = -1.5, font = 2)
  }
})
page({
  fs <- both("base_content.txt")
  if (length(fs)) {
    par(mfrow = c(1, length(fs)))
    cols <- c(A = "green3", T = "red", C = "blue", G = "black", N = "grey50")
    for (f in fs) {
      t <- content(f); t <- t[t$kind != "GC", ]
      plot(NA, xlim = c(0, 100), ylim = c(0, max(t$n) / 1e3), xlab = "share of the read (%)", ylab = "reads (thousands)", main = label(f))
      for (k in names(cols)) { x <- t[t$kind == k, ]; if (nrow(x)) lines(x$pct, x$n / 1e3, col = cols[k]) }
      legend("topright", legend = names(cols), col = cols, lty = 1, bty = "n")
    }
    par(mfrow = c(1, 1))
    mtext("Nucleotide content of the reads", outer = TRUE, line = -1.5, font = 2)
  }
})

# 4. composition per cycle (position x A, T, C, G, N), then N alone
base_matrix <- function(f) { m <- as.matrix(read.table(f, header = FALSE)); colnames(m) <- c("A", "T", "C", "G", "N"); m }
page({
  fs <- both("base.matrix")
  if (length(fs)) {
    par(mfrow = c(1, length(fs)))
    cols <- c(A = "green3", T = "red", C = "blue", G = "black")
    for (f in fs) {
      m <- base_matrix(f); pct <- 100 * m / pmax(1, rowSums(m))
      plot(NA, xlim = c(1, nrow(m)), ylim = c(0, max(50, pct[, 1:4])), xlab = "cycle", ylab = "%", main = label(f))
      for (k in names(cols)) lines(seq_len(nrow(m)), pct[, k], col = cols[k])
      legend("topright", legend = names(cols), col = cols, lty = 1, bty = "n")
    }
    par(mfrow = c(1, 1))
    mtext("Nucleotide content per cycle", outer = TRUE, line = -1.5, font = 2)
  }
})
page({
  fs <- both("base.matrix")
  if (length(fs)) {
    par(mfrow = c(1, length(fs)))
    for (f in fs) {
      m <- base_matrix(f)
      plot(seq_len(nrow(m)), 100 * m[, "N"] / pmax(1, rowSums(m)), type = "h", xlab = "cycle", ylab = "N (%)", main = label(f), col = "grey30")
    }
    par(mfrow = c(1, 1))
    mtext("N content per cycle", outer = TRUE, line = -1.5, font = 2)
  }
})

# 5. k-mers: rarefaction curve and count histogram
page({
  f <- post("Kmercount.txt")
  if (have(f)) {
    t <- read.table(f, header = FALSE, col.names = c("reads", "distinct", "total"))
    x <- cumsum(t$reads)
    plot(x / 1e6, t$distinct / 1e6, type = "b", xlab = "reads sampled (millions)", ylab = "distinct k-mers (millions)", main = "K-mer rarefaction curve")
    if (nrow(t) > 1) {
      legend("bottomright", legend = sprintf("last slope %.3f distinct k-mers per read", diff(tail(t$distinct, 2)) / diff(tail(x, 2))), bty = "n")
    }
  }
})
page({
  f <- post("kmerH.txt")
  if (have(f)) {
    t <- read.table(f, header = FALSE, col.names = c("count", "kmers"))
    t <- t[order(t$count), ]
    plot(t$count, t$kmers, log = "xy", type = "h", xlab = "occurrences of a k-mer", ylab = "k-mers", main = "K-mer frequency histogram")
  }
})

# 6. average read quality
page({
  fs <- both("for_qual_histogram.txt")
  if (length(fs)) {
    par(mfrow = c(1, length(fs)))
    for (f in fs) {
      t <- read.table(f, header = TRUE)
      t <- t[order(t$Score), ]
      barplot(t$readsNum / 1e6, names.arg = t$Score, xlab = "average quality of a read", ylab = "reads (millions)", main = label(f), border = NA, col = "orange3")
    }
    par(mfrow = c(1, 1))
    mtext("Average read quality histogram", outer = TRUE, line = -1.5, font = 2)
  }
})

# 7. quality per cycle from the position x score matrix: box plot, surface, totals per score
quality_matrix <- function(f) as.matrix(read.table(f, header = FALSE))
quantile_row <- function(r, probs) { cs <- cumsum(r); tot <- cs[length(cs)]; if (tot == 0) return(rep(NA, length(probs))); sapply(probs, function(p) which(cs >= p * tot)[1] - 1) }
page({
  fs <- both("quality.matrix")
  if (length(fs)) {
    par(mfrow = c(1, length(fs)))
    for (f in fs) {
      m <- quality_matrix(f)
      st <- apply(m, 1, quantile_row, probs = c(0.1, 0.25, 0.5, 0.75, 0.9))
      z <- list(stats = st, n = rowSums(m), conf = matrix(NA_real_, 2, ncol(st)), out = numeric(0), group = numeric(0), names = seq_len(ncol(st)))
      bxp(z, outline = FALSE, xlab = "cycle", ylab = "quality", main = label(f), ylim = c(0, ncol(m) - 1), boxfill = "khaki", whisklty = 1, xaxt = "n")
      at <- pretty(seq_len(ncol(st))); at <- at[at >= 1 & at <= ncol(st)]
      axis(1, at = at, labels = at)
      lines(seq_len(ncol(st)), (m %*% (0:(ncol(m) - 1))) / pmax(1, rowSums(m)), col = "red")
    }
    par(mfrow = c(1, 1))
    mtext("Quality per cycle (10 / 25 / 50 / 75 / 90 % and the mean)", outer = TRUE, line = -1.5, font = 2)
  }
})
page({
  fs <- both("quality.matrix")
  if (length(fs)) {
    par(mfrow = c(1, length(fs)))
    for (f in fs) {
      m <- quality_matrix(f)
      persp(seq_len(nrow(m)), 0:(ncol(m) - 1), m / 1e3, theta = 40, phi = 25, xlab = "cycle", ylab = "quality", zlab = "bases (thousands)",
            main = label(f), col = "lightblue", border = NA, shade = 0.5, ticktype = "detailed")
    }
    par(mfrow = c(1, 1))
    mtext("Quality surface (cycle x score x bases)", outer = TRUE, line = -1.5, font = 2)
  }
})
page({
  fs <- both("quality.matrix")
  if (length(fs)) {
    par(mfrow = c(1, length(fs)))
    for (f in fs) {
      m <- quality_matrix(f); n <- colSums(m)
      q20 <- 100 * sum(n[21:length(n)]) / max(1, sum(n)); q30 <- 100 * sum(n[31:length(n)]) / max(1, sum(n))
      barplot(n / 1e6, names.arg = 0:(length(n) - 1), xlab = "quality", ylab = "bases (millions)", main = label(f), border = NA,
              col = ifelse(0:(length(n) - 1) >= 30, "darkgreen", ifelse(0:(length(n) - 1) >= 20, "orange", "red3")))
      legend("topleft", legend = c(sprintf(">= Q20: %.2f %%", q20), sprintf(">= Q30: %.2f %%", q30)), bty = "n")
    }
    par(mfrow = c(1, 1))
    mtext("Bases per quality score", outer = TRUE, line = -1.5, font = 2)
  }
})

invisible(dev.off())
quit(save = "no")
)R";
    return s;
}

// A helper process forked BEFORE the first HIP call (a process that has initialised the GPU must not exec): it waits for the
// script on a pipe and then runs R exactly as the reference does.  An empty script (--trim_only, or a run that failed) = no R.
struct ReportHelper {
    pid_t pid = -1;
    int fd = -1;
    void start()
    {
        int pf[2];
        if (pipe(pf) != 0) return;
        fflush(nullptr);
        pid = fork();
        if (pid < 0) { close(pf[0]); close(pf[1]); pid = -1; return; }
        if (pid == 0) {
            close(pf[1]);
            // the script arrives behind its length: a parent that died half way through must not make R run half a script
            uint64_t want = 0;
            std::string script;
            char buf[65536];
            ssize_t n;
            size_t got = 0;
            while (got < sizeof want && (n = read(pf[0], (char *)&want + got, sizeof want - got)) > 0) got += (size_t)n;
            if (got == sizeof want) while ((n = read(pf[0], buf, sizeof buf)) > 0) script.append(buf, (size_t)n);
            close(pf[0]);
            if (got != sizeof want || want == 0) _exit(0); // (no report wanted: --trim_only decided later, or the run failed)
            if (script.size() != want) { fprintf(stderr, "Warning: Unable to run R for plot generation\n"); _exit(1); }
            FILE *r = popen("R --vanilla --silent --slave", "w"); // plot.cpp:507
            if (!r) { fprintf(stderr, "Warning: Unable to run R for plot generation\n"); _exit(1); }
            const bool ok = fwrite(script.data(), 1, script.size(), r) == script.size();
            const int rc = pclose(r);
            _exit(ok && rc == 0 ? 0 : 1);
        }
        close(pf[0]);
        fd = pf[1];
    }
    // hands the script over and waits until R is done with the tables
    void run(const std::string &script)
    {
        if (pid < 0) return;
        const uint64_t len = script.size();
        std::string msg((const char *)&len, sizeof len);
        msg += script;
        size_t off = 0;
        while (off < msg.size()) { const ssize_t n = write(fd, msg.data() + off, msg.size() - off); if (n <= 0) break; off += (size_t)n; } // (SIGPIPE is ignored: a dead helper = EPIPE)
        close(fd); fd = -1;
        int st = 0;
        waitpid(pid, &st, 0);
        pid = -1;
        if (off != msg.size()) fprintf(stderr, "Warning: Unable to run R for plot generation\n"); // (the helper says so itself when popen or R fails, as plot.cpp:507-513 does)
    }
};

std::vector<std::string> table_files(const Opt &o)
{
    std::vector<std::string> v;
    const std::string d = o.output_dir + "/", p = o.prefix;
    for (const char *n : {"quality.matrix", "base.matrix", "for_qual_histogram.txt", "base_content.txt", "length_count.txt"}) {
        v.push_back(d + "qa." + p + "." + n);
        v.push_back(d + p + "." + n);
    }
    v.push_back(d + p + ".kmerH.txt");
    v.push_back(d + p + ".Kmercount.txt");
    return v;
}
} // namespace
