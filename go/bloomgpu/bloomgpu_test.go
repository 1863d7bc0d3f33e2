package bloomgpu

import (
	"fmt"
	"testing"
)

// The public MurmurHash3_x64_128 vector for "hello" (seed 0) through bsg_hash_entries: h0, h1 of bloom/v3's
// baseHashes are exactly that digest.  Needs a gfx950 device; skipped otherwise.
func TestHashEntriesPublicVector(t *testing.T) {
	g, err := Open([]int32{0})
	if err != nil {
		t.Skip(err)
	}
	defer g.Close()
	bytes, off := PackEntries([]string{"hello", ""})
	h, err := g.HashEntries(bytes, off)
	if err != nil {
		t.Fatal(err)
	}
	if h[0][0] != 0xcbd8a7b341bd9b02 || h[0][1] != 0x5b1e906a48ae1d19 {
		t.Fatalf("murmur3(hello) = %016x %016x", h[0][0], h[0][1])
	}
	if h[1][0] != 0 || h[1][1] != 0 {
		t.Fatalf("murmur3(\"\") = %016x %016x", h[1][0], h[1][1])
	}
}

func TestEstimateParameters(t *testing.T) {
	for _, c := range []struct {
		n    uint64
		p    float64
		m, k uint64
	}{{100, 0.01, 959, 7}, {1, 0.001, 15, 11}, {20000, 0.001, 287552, 10}} {
		m, k, err := EstimateParameters(c.n, c.p)
		if err != nil || m != c.m || k != c.k {
			t.Fatalf("EstimateParameters(%d, %g) = %d, %d, %v", c.n, c.p, m, k, err)
		}
	}
}

// A failing call's message is read back from the scope it was made on, from another goroutine.
func TestScopesOwnTheirErrors(t *testing.T) {
	g, err := Open([]int32{0})
	if err != nil {
		t.Skip(err)
	}
	defer g.Close()
	a, _ := g.Scope()
	b, _ := g.Scope()
	defer a.Close()
	defer b.Close()
	errA := a.ArenaFree(Arena{ID: 0xDEAD})
	errB := b.BatchFree(Batch{ID: 0xBEEF})
	done := make(chan [2]string)
	go func() { done <- [2]string{errA.Error(), errB.Error()} }()
	got := <-done
	if got[0] == got[1] || errA == nil || errB == nil {
		t.Fatalf("scopes share an error slot: %q / %q", got[0], got[1])
	}
}

// Tokenizer.Func is strings.FieldsFunc(lowered, isSep); Validate refuses NUL and non-ASCII separators.  Host only.
func TestTokenizerFunc(t *testing.T) {
	punct := Tokenizer{Separators: " \t\n\v\f\r,;:=/.-\"[]()", UnicodeSpace: true, Lower: true}
	cases := []struct {
		tok  Tokenizer
		in   string
		want []string
	}{
		{punct, "user=Alice GET /api/v1/users", []string{"user", "alice", "get", "api", "v1", "users"}},
		{punct, "-1.5E-3", []string{"1", "5e", "3"}},
		{Tokenizer{Separators: " \t\n\v\f\r,;:=/.-\"[]()", UnicodeSpace: true}, "-1.5E-3", []string{"1", "5E", "3"}},
		{Tokenizer{Separators: "k", Lower: true}, "xKy", []string{"x", "y"}},
		{Tokenizer{Separators: " "}, "a\u00a0b c", []string{"a\u00a0b", "c"}},
		{Tokenizer{Separators: " \t\n\v\f\r", UnicodeSpace: true, Lower: true}, "Hello  World\u3000X", []string{"hello", "world", "x"}},
	}
	for _, c := range cases {
		got := c.tok.Func()(c.in)
		if fmt.Sprint(got) != fmt.Sprint(c.want) {
			t.Errorf("%+v(%q) = %q, want %q", c.tok, c.in, got, c.want)
		}
	}
	if got := (Tokenizer{Separators: "é,"}).Func()("a,b"); fmt.Sprint(got) != "[a b]" { // an unvalidated spec must not panic
		t.Errorf("Func with a non-ASCII separator: %q", got)
	}
	for _, bad := range []string{"\x00", "é", "a\u3000"} {
		if (Tokenizer{Separators: bad}).Validate() == nil {
			t.Errorf("Validate(%q) accepted", bad)
		}
	}
}

// IngestRowsTok / MatchRowsTok: Token("alice") finds {"msg":"user=alice"} under the punctuation tokenizer only.  Needs a gfx950
// device; skipped otherwise.
func TestMatchRowsTokPunctuation(t *testing.T) {
	g, err := Open([]int32{0})
	if err != nil {
		t.Skip(err)
	}
	defer g.Close()
	row := []byte(`{"msg":"user=alice"}`)
	off := []uint64{0, uint64(len(row))}
	conds := []MatchCond{{Kind: KindToken, Token: "alice"}}
	prog := []uint32{0}
	punct := Tokenizer{Separators: " \t\n\v\f\r,;:=/.-\"[]()", UnicodeSpace: true, Lower: true}
	bits, host, err := g.MatchRowsTok(row, off, conds, prog, punct)
	if err != nil || len(host) != 0 || bits[0]&1 != 1 {
		t.Fatalf("punctuation: bits %v host %v err %v", bits, host, err)
	}
	bits, _, err = g.MatchRows(row, off, conds, prog)
	if err != nil || bits[0]&1 != 0 {
		t.Fatalf("default: bits %v err %v", bits, err)
	}
	in, err := g.IngestRowsTok(row, off, []uint32{0, 1}, nil, 0, 0, punct)
	if err != nil {
		t.Fatal(err)
	}
	defer in.Free()
	counts, _, err := in.Finish()
	if err != nil || counts[0] != 1 || counts[1] != 2 || counts[2] != 2 {
		t.Fatalf("counts %v err %v", counts, err)
	}
}
